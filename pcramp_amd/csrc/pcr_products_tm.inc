// Products of a primer pool with the Tm of their two sites, Tm-floored, and the pool's amplification bitsets at that floor
// (pcr_pool_products_tm; included by pcr_device.hip after pcr_site_tm.inc, whose kernels it launches as they are).
//
// pcr_pool_products and pcr_site_tm enumerate the same (entry, oligo) items with the same kernel, and k_pool_join forms a product
// from two item indices: with the site's tm_max stored per ITEM, a product's two Tm are two array reads and no lookup is made.
//   1. k_pool_entry_oligos<false> / <true> (pcr_pool.inc) + a scan: the items and item_off.
//   2. k_site_jobs + a scan, k_site_tm (pcr_site_tm.inc): one wave per (item, expansion) -> res[job].
//   3. k_item_tm: a thread per item walks its expansions in index order (strict >: the lowest index wins, no float atomics) ->
//      item_tm[k] = {tm_max, NO_TM}.  Indexed by item; the sites are never sorted.
//   4. k_products_join<false> / <true>: k_pool_join's geometry, the same tests in the same order, plus the floor on
//      min(item_tm[k], item_tm[t]).  The count pass also sets the bits: a kept product whose (plus, minus) is a pool pair in
//      either orientation ORs bit `sequence` into that pair's row with a 64-bit atomicOr (many threads set the same bit and the
//      same word: the atomic is what makes that exact).  The emit pass writes the 48-byte records and their (begin, end) keys.
//   5. The record order as in pcr_pool_products: two stable radix sorts and a gather that sets `intended`.
// With tm_floor <= 0, cap = 0 and no bitset, steps 2 and 3 are skipped and the join only counts: pcr_pool_products' count.
// The call owns its scratch (pcr_ctx::ptm_*); the dG table is the handle's (th_dg, keyed by its salt as for every thermo call).

namespace {

struct alignas(8) ItemTm { float tm; uint32_t no_tm; };                        // tm_max of the item's site (0 with NO_TM) and its NO_TM bit: one 8-byte load
struct ProductPair { uint32_t key, fr_row, rf_row, pad; };                      // key = plus*n_ol + minus -> the rows of the first pool pair (F, R) / (R, F) that it is
constexpr uint32_t PTM_NO_ROW = 0xFFFFFFFFu;

// Item k: its expansions joff[k] .. joff[k + 1] - 1 in index order; the highest Tm (k_site_reduce's rule for tm_max).
__global__ __launch_bounds__(POOL_THREADS) void k_item_tm(const uint64_t *__restrict__ joff, uint32_t n_items, const float4 *__restrict__ res,
	ItemTm *__restrict__ item_tm, uint32_t *__restrict__ error)
{
	const uint32_t k = blockIdx.x*blockDim.x + threadIdx.x;
	if(k >= n_items) return;
	const uint64_t j0 = joff[k], j1 = joff[k + 1];
	float tm = 0.0f;
	uint32_t st = 0;
	for(uint64_t j = j0;j < j1;++j){
		const float4 v = res[j];
		st |= __float_as_uint(v.w);
		if(j == j0 || v.x > tm) tm = v.x;
	}
	ItemTm r;
	r.no_tm = (st & SITE_ST_NO_TM) ? 1u : 0u;
	r.tm = r.no_tm ? 0.0f : tm;
	if(st & SITE_ST_ERROR) atomicOr(error, 1u);
	item_tm[k] = r;
}

// k_pool_join with the two sites' Tm: one thread per item k, a plus-strand item (i, x) against the minus-strand items (j, y) of
// its segment.  item_tm = NULL: no Tm is read and nothing is floored (the plain count).  <false>: count[k], and with bits != NULL
// the bit of every kept product of a pool pair; <true>: records, (begin, end) sort keys and identity indices at rec_off[k] ..
template<bool EMIT>
__global__ __launch_bounds__(POOL_THREADS) void k_products_join(const DevEntry *__restrict__ db, uint32_t cap, const uint32_t *__restrict__ touched,
	const uint32_t *__restrict__ seg_hi, const uint2 *__restrict__ items, uint32_t n_items, const uint64_t *__restrict__ item_off,
	const PoolOligo *__restrict__ oligos, uint32_t n_ol, const uint4 *__restrict__ planes, const uint64_t *__restrict__ blk_off,
	const uint64_t *__restrict__ len, const uint8_t *__restrict__ has_eos, int32_t amp_min, int32_t amp_max,
	const ItemTm *__restrict__ item_tm, float tm_floor, const uint32_t *__restrict__ intended, const ProductPair *__restrict__ pair_tab,
	uint32_t n_tab, unsigned long long *__restrict__ bits, uint32_t n_pool, uint32_t words,
	uint32_t *__restrict__ count, const uint64_t *__restrict__ rec_off, pcr_product_tm *__restrict__ rec, uint64_t *__restrict__ key,
	uint32_t *__restrict__ ord)
{
	__shared__ int2 ss[POOL_MAX_OLIGOS];                                        // Word::start() / stop()
	for(uint32_t o = threadIdx.x;o < n_ol;o += blockDim.x) ss[o] = make_int2(oligos[o].start, oligos[o].stop);
	__syncthreads();
	const uint32_t k = blockIdx.x*blockDim.x + threadIdx.x;
	if(k >= n_items) return;
	const uint2 it = items[k];
	const uint32_t g = it.x, x = it.y;
	const uint32_t i = touched[g/cap]*cap + g % cap;
	const DevEntry ei = db[i];
	uint32_t c = 0;
	uint64_t w = EMIT ? rec_off[k] : 0;
	if(ei.strand == 1){
		const uint32_t hi = seg_hi[ei.seq];
		const int32_t L = (int32_t)len[ei.seq];
		const uint64_t blk_base = blk_off[ei.seq];
		const bool eos = has_eos[ei.seq] != 0;
		const int2 P = ss[x];
		const int32_t p5 = ei.loc + P.x, p3 = ei.loc + P.y;                      // template_loc5/3, sequence.h:57-75
		ItemTm tp; tp.tm = 0.0f; tp.no_tm = 0;
		if(item_tm) tp = item_tm[k];
		const bool floored = item_tm && tm_floor > 0.0f;
		if(!(floored && tp.tm < tm_floor)){                                      // (a plus site below the floor keeps no product)
			for(uint32_t j = i + 1;j < hi;++j){
				const DevEntry ej = db[j];
				if(ej.loc - ei.loc > amp_max + 128) break;
				if(ej.strand != 2) continue;
				const uint32_t gj = g + (j - i);                                     // same segment: consecutive DB threads
				const uint64_t t_end = item_off[gj + 1];
				for(uint64_t t = item_off[gj];t < t_end;++t){
					const uint32_t y = items[t].y;
					const int2 M = ss[y];
					const int32_t m5 = ej.loc - M.y, m3 = ej.loc - M.x;
					if(p3 >= m5) continue;                                           // pcr_assay.cpp:468-471
					const int32_t amp_len = m3 - p5 + 1;
					if(amp_len < amp_min || amp_len > amp_max) continue;             // :477-484
					const int32_t in_start = p3 + 1 - 4;                             // :489-490
					const int32_t in_len = m5 - in_start + 8;                        // :492-494
					if(in_start < 0 || in_len < 0 || in_start + in_len > L) continue;
					if(eos && has_split(planes, blk_base, in_start, in_len)) continue;   // :504-521
					ItemTm tm; tm.tm = 0.0f; tm.no_tm = 0;
					if(item_tm) tm = item_tm[t];
					if(floored && !(((tp.tm < tm.tm) ? tp.tm : tm.tm) >= tm_floor)) continue;   // min(tm_plus, tm_minus) >= tm_floor
					if(EMIT){
						pcr_product_tm r;
						r.plus_oligo = x; r.minus_oligo = y; r.sequence = ei.seq; r.begin = p5; r.end = m3;
						r.inner_start = in_start; r.inner_length = in_len; r.intended = 0;
						r.tm_plus = tp.tm; r.tm_minus = tm.tm;
						r.flags = (tp.no_tm ? PCR_PRODUCT_PLUS_NO_TM : 0u) | (tm.no_tm ? PCR_PRODUCT_MINUS_NO_TM : 0u);
						r.reserved = 0;
						rec[w] = r;
						key[w] = ((uint64_t)((uint32_t)p5 ^ 0x80000000u) << 32) | ((uint32_t)m3 ^ 0x80000000u);   // signed order
						ord[w] = (uint32_t)w;
						++w;
					}
					else{
						++c;
						const uint32_t b = x*n_ol + y;
						if(bits && ((intended[b >> 5] >> (b & 31)) & 1u)){
							uint32_t lo = 0, above = n_tab;                              // pair_tab[lo].key <= b < pair_tab[above].key; an intended b is in the table
							while(above - lo > 1u){
								const uint32_t mid = lo + (above - lo)/2u;
								if(pair_tab[mid].key <= b) lo = mid; else above = mid;
							}
							const ProductPair pp = pair_tab[lo];
							if(pp.key == b){
								const unsigned long long bit = 1ull << (ei.seq & 63u);
								const size_t word = ei.seq >> 6;
								if(pp.fr_row != PTM_NO_ROW) atomicOr(bits + (size_t)pp.fr_row*words + word, bit);
								if(pp.rf_row != PTM_NO_ROW) atomicOr(bits + ((size_t)n_pool + pp.rf_row)*words + word, bit);
							}
						}
					}
				}
			}
		}
	}
	if(!EMIT) count[k] = c;
}

// (plus_oligo, minus_oligo, sequence) of the records in their (begin, end) order
__global__ void k_products_key2(const pcr_product_tm *__restrict__ rec, const uint32_t *__restrict__ ord, uint32_t n, uint32_t seq_bits,
	uint32_t oligo_bits, uint64_t *__restrict__ key)
{
	const uint32_t r = blockIdx.x*blockDim.x + threadIdx.x;
	if(r >= n) return;
	const uint32_t at = ord[r];
	const uint32_t plus = rec[at].plus_oligo, minus = rec[at].minus_oligo, seq = rec[at].sequence;
	key[r] = ((uint64_t)plus << (oligo_bits + seq_bits)) | ((uint64_t)minus << seq_bits) | seq;
}

__global__ void k_products_gather(const pcr_product_tm *__restrict__ rec, const uint32_t *__restrict__ ord, uint32_t n,
	const uint32_t *__restrict__ intended, uint32_t n_ol, pcr_product_tm *__restrict__ out)
{
	const uint32_t r = blockIdx.x*blockDim.x + threadIdx.x;
	if(r >= n) return;
	pcr_product_tm p = rec[ord[r]];
	const uint32_t b = p.plus_oligo*n_ol + p.minus_oligo;
	p.intended = (intended[b >> 5] >> (b & 31)) & 1u;
	out[r] = p;
}

} // namespace

extern "C" {

int64_t pcr_pool_products_tm(pcr_ctx *ctx, pcr_set which, const pcr_pair *pool, uint32_t n_pool, float threshold,
	int32_t amp_min, int32_t amp_max, const pcr_thermo_args *args, float template_strand, float tm_floor,
	uint32_t *oligo_id, pcr_product_tm *out, uint64_t cap, uint64_t *bits_fr, uint64_t *bits_rf)
{
	static_assert(sizeof(pcr_product_tm) == 48, "record layout");
	static_assert(sizeof(ItemTm) == 8 && sizeof(ProductPair) == 16, "table layout");
	static_assert((uint64_t)POOL_MAX_OLIGOS*POOL_MAX_OLIGOS <= 0xFFFFFFFFull, "a (plus, minus) key is 32-bit");
	// ---- the arguments, before the handle (pcr_site_tm's checks in its order, then the floor)
	if(!set_ok(which)){ g_err = "pcr_pool_products_tm: unknown sequence set"; return PCR_ERR_ARG; }
	if(which != PCR_SET_TARGET && which != PCR_SET_BACKGROUND){ g_err = "pcr_pool_products_tm: PCR_SET_MULTIPLEX is not supported (PCR_SET_TARGET or PCR_SET_BACKGROUND)"; return PCR_ERR_ARG; }
	if(!args || (n_pool && (!pool || !oligo_id)) || (cap && !out)){ g_err = "pcr_pool_products_tm: bad argument"; return PCR_ERR_ARG; }
	if(n_pool > PCR_POOL_MAX_PAIRS){ g_err = "pcr_pool_products_tm: pool larger than PCR_POOL_MAX_PAIRS"; return PCR_ERR_ARG; }
	if(!(template_strand >= 0.0f) || !(args->primer_strand >= 0.0f)){ g_err = "pcr_pool_products_tm: negative strand concentration (NucCruc::strand, nuc_cruc.h:818-826)"; return PCR_ERR_ARG; }
	if(!(args->salt >= 1.0e-6f && args->salt <= 1.0f)){ g_err = "pcr_pool_products_tm: salt outside [1e-6, 1] (NucCruc::salt, nuc_cruc.h:780-788)"; return PCR_ERR_ARG; }
	// the distinct oligos, in order of first appearance (as pcr_pool_products and pcr_site_tm)
	std::vector<PoolOligo> ol;
	std::vector<SiteOligoX> olx;
	std::map<std::pair<uint64_t, uint64_t>, uint32_t> id_of;
	const float thr2 = threshold*threshold;                                      // pcr_assay.cpp:775-776
	for(uint32_t s = 0;s < 2*n_pool;++s){
		const pcr_word128 &wd = (s & 1) ? pool[s/2].r : pool[s/2].f;
		auto ins = id_of.insert(std::make_pair(std::make_pair(wd.w[0], wd.w[1]), (uint32_t)ol.size()));
		if(ins.second){
			OligoDev d; fill_oligo(d, wd.w, thr2);
			const uint32_t occ = pcrhost::planes_occupied(d.m);
			if(!occ || __builtin_popcount(occ) != d.stop - d.start + 1){
				g_err = "pcr_pool_products_tm: an oligo is empty or has a hole between its ends (NucCruc::set_query throws)"; return PCR_ERR_ARG;
			}
			const double degen = pcrhost::planes_degeneracy(d.m);
			if(degen > (double)PCR_SITE_MAX_EXPANSIONS){ g_err = "pcr_pool_products_tm: an oligo has more than PCR_SITE_MAX_EXPANSIONS expansions"; return PCR_ERR_ARG; }
			PoolOligo p; p.m = d.m; p.floor2 = d.floor2; p.start = d.start; p.stop = d.stop; p.pad = 0;
			ol.push_back(p);
			const float ca = (float)(args->primer_strand/degen), cb = template_strand;
			const float strand = (ca > cb) ? ca - 0.5f*cb : cb - 0.5f*ca;          // nuc_cruc.h:832-837
			if(!(strand > 0.0f)){ g_err = "pcr_pool_products_tm: the strand concentration of an oligo's duplex is zero (primer_strand / degeneracy and template_strand both 0)"; return PCR_ERR_ARG; }
			SiteOligoX x; x.n_exp = (uint32_t)degen;
			x.log_strand = logf(strand);
			olx.push_back(x);
		}
		oligo_id[s] = ins.first->second;
	}
	if(!std::isfinite(tm_floor)){ g_err = "pcr_pool_products_tm: tm_floor is not finite"; return PCR_ERR_ARG; }
	if(!ctx){ g_err = "pcr_pool_products_tm: null handle"; return PCR_ERR_ARG; }
	{ const int drc = drain(ctx); if(drc != PCR_OK) return drc; }
	HIP_TRY(hipSetDevice(ctx->device));
	SeqSet &S = ctx->sets[which];
	if(!S.have_db){ g_err = "pcr_pool_products_tm: no word DB (call pcr_select_words or pcr_select_sites first)"; return PCR_ERR_STATE; }
	if(n_pool == 0) return 0;
	const uint32_t words = (uint32_t)((S.n + 63)/64);
	const size_t row_words = (size_t)n_pool*words;
	const bool want_bits = bits_fr || bits_rf;
	// whatever the count, the rows asked for are written in full
	auto zero_rows = [&](){
		if(bits_fr) memset(bits_fr, 0, row_words*sizeof(uint64_t));
		if(bits_rf) memset(bits_rf, 0, row_words*sizeof(uint64_t));
	};
	{ const int erc = ensure_touched(ctx, S); if(erc != PCR_OK) return erc; }
	if(S.n_entries == 0 || S.n_touched == 0){ zero_rows(); return 0; }
	const uint32_t n_ol = (uint32_t)ol.size();
	const bool melt = tm_floor > 0.0f || cap > 0 || want_bits;                   // else: pcr_pool_products' count, no DP
	// the intended bitmap, and (plus, minus) -> the rows of the first pool pair that is (F, R) = (plus, minus) / (R, F) = (plus, minus)
	std::vector<uint32_t> intended(((size_t)n_ol*n_ol + 31)/32, 0);
	std::map<uint32_t, ProductPair> tab_of;
	for(uint32_t i = 0;i < n_pool;++i){
		const uint32_t f = oligo_id[2*i], r = oligo_id[2*i + 1];
		for(uint32_t b : {f*n_ol + r, r*n_ol + f}) intended[b >> 5] |= 1u << (b & 31);
		for(int o = 0;o < 2;++o){
			const uint32_t b = o ? r*n_ol + f : f*n_ol + r;
			ProductPair fresh; fresh.key = b; fresh.fr_row = fresh.rf_row = PTM_NO_ROW; fresh.pad = 0;
			ProductPair &pp = tab_of.insert(std::make_pair(b, fresh)).first->second;
			uint32_t &row = o ? pp.rf_row : pp.fr_row;
			if(row == PTM_NO_ROW) row = i;
		}
	}
	std::vector<ProductPair> tab;
	tab.reserve(tab_of.size());
	for(const auto &kv : tab_of) tab.push_back(kv.second);                       // (key order)
	int rc;
	const size_t ol_bytes = ol.size()*sizeof(PoolOligo), tab_bytes = tab.size()*sizeof(ProductPair), olx_bytes = olx.size()*sizeof(SiteOligoX),
		int_bytes = intended.size()*sizeof(uint32_t);
	std::vector<uint8_t> blob(ol_bytes + tab_bytes + olx_bytes + int_bytes);     // 32-, 16-, 8- and 4-byte records, in that order: each is aligned
	memcpy(blob.data(), ol.data(), ol_bytes);
	memcpy(blob.data() + ol_bytes, tab.data(), tab_bytes);
	memcpy(blob.data() + ol_bytes + tab_bytes, olx.data(), olx_bytes);
	memcpy(blob.data() + ol_bytes + tab_bytes + olx_bytes, intended.data(), int_bytes);
	if((rc = ctx->ptm_in.ensure(blob.size())) != PCR_OK) return rc;
	const PoolOligo *d_ol = (const PoolOligo *)ctx->ptm_in.p;
	const ProductPair *d_tab = (const ProductPair *)(ctx->ptm_in.p + ol_bytes);
	const SiteOligoX *d_olx = (const SiteOligoX *)(ctx->ptm_in.p + ol_bytes + tab_bytes);
	const uint32_t *d_intended = (const uint32_t *)(ctx->ptm_in.p + ol_bytes + tab_bytes + olx_bytes);
	HIP_TRY(hipMemcpyAsync(ctx->ptm_in.p, blob.data(), blob.size(), hipMemcpyHostToDevice, ctx->stream));
	// ---- 1. the items (k_pool_entry_oligos: count, scan, fill)
	const uint32_t n_db = S.n_touched*S.db_cap;
	if((rc = ctx->ptm_cnt.ensure((size_t)n_db + 1)) != PCR_OK) return rc;
	if((rc = ctx->ptm_eoff.ensure((size_t)n_db + 1)) != PCR_OK) return rc;
	HIP_TRY(hipMemsetAsync(ctx->ptm_cnt.p + n_db, 0, sizeof(uint32_t), ctx->stream));
	size_t tmp = 0;
	HIP_TRY(rocprim::exclusive_scan(nullptr, tmp, ctx->ptm_cnt.p, ctx->ptm_eoff.p, uint64_t(0), (size_t)n_db + 1, rocprim::plus<uint64_t>(), ctx->stream));
	if((rc = ctx->ptm_tmp.ensure(tmp + 16)) != PCR_OK) return rc;
	const unsigned grid_e = std::min<unsigned>((n_db + POOL_THREADS - 1)/POOL_THREADS, ctx->n_cu*8);
	hipLaunchKernelGGL(k_pool_entry_oligos<false>, dim3(grid_e), dim3(POOL_THREADS), 0, ctx->stream, S.db.p, n_db, S.db_cap, S.touched.p,
		S.d_seg_hi, S.d_active.p, d_ol, n_ol, ctx->ptm_cnt.p, (const uint64_t *)nullptr, (uint2 *)nullptr);
	HIP_TRY(hipGetLastError());
	HIP_TRY(rocprim::exclusive_scan(ctx->ptm_tmp.p, tmp, ctx->ptm_cnt.p, ctx->ptm_eoff.p, uint64_t(0), (size_t)n_db + 1, rocprim::plus<uint64_t>(), ctx->stream));
	uint64_t n_items = 0;
	HIP_TRY(hipMemcpyAsync(&n_items, ctx->ptm_eoff.p + n_db, sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
	HIP_TRY(hipStreamSynchronize(ctx->stream));                                   // (blob is read by now)
	if(n_items >= POOL_MAX_ITEMS){ g_err = "pcr_pool_products_tm: too many (entry, oligo) hits"; return PCR_ERR_CAPACITY; }
	if(n_items == 0){ zero_rows(); return 0; }
	if((rc = ctx->ptm_items.ensure(n_items)) != PCR_OK) return rc;
	hipLaunchKernelGGL(k_pool_entry_oligos<true>, dim3(grid_e), dim3(POOL_THREADS), 0, ctx->stream, S.db.p, n_db, S.db_cap, S.touched.p,
		S.d_seg_hi, S.d_active.p, d_ol, n_ol, (uint32_t *)nullptr, (const uint64_t *)ctx->ptm_eoff.p, ctx->ptm_items.p);
	HIP_TRY(hipGetLastError());
	const uint32_t ni = (uint32_t)n_items;
	const unsigned grid_i = (ni + POOL_THREADS - 1)/POOL_THREADS;
	if((rc = ctx->ptm_cnt.ensure((size_t)ni + 1)) != PCR_OK) return rc;         // (the entry counts are spent)
	if((rc = ctx->ptm_flag.ensure(1)) != PCR_OK) return rc;
	HIP_TRY(hipMemsetAsync(ctx->ptm_flag.p, 0, sizeof(uint32_t), ctx->stream));
	const ItemTm *d_item_tm = nullptr;
	if(melt){
		// ---- 2. job offsets, the jobs (k_site_jobs, k_site_tm as they stand)
		if((rc = ctx->ptm_joff.ensure((size_t)ni + 1)) != PCR_OK) return rc;
		HIP_TRY(hipMemsetAsync(ctx->ptm_cnt.p + ni, 0, sizeof(uint32_t), ctx->stream));
		hipLaunchKernelGGL(k_site_jobs, dim3(grid_i), dim3(POOL_THREADS), 0, ctx->stream, (const uint2 *)ctx->ptm_items.p, ni, d_olx, ctx->ptm_cnt.p);
		HIP_TRY(hipGetLastError());
		tmp = 0;
		HIP_TRY(rocprim::exclusive_scan(nullptr, tmp, ctx->ptm_cnt.p, ctx->ptm_joff.p, uint64_t(0), (size_t)ni + 1, rocprim::plus<uint64_t>(), ctx->stream));
		if((rc = ctx->ptm_tmp.ensure(tmp + 16)) != PCR_OK) return rc;
		HIP_TRY(rocprim::exclusive_scan(ctx->ptm_tmp.p, tmp, ctx->ptm_cnt.p, ctx->ptm_joff.p, uint64_t(0), (size_t)ni + 1, rocprim::plus<uint64_t>(), ctx->stream));
		uint64_t n_jobs64 = 0;
		HIP_TRY(hipMemcpyAsync(&n_jobs64, ctx->ptm_joff.p + ni, sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
		HIP_TRY(hipStreamSynchronize(ctx->stream));
		if(n_jobs64 >= POOL_MAX_ITEMS){ g_err = "pcr_pool_products_tm: too many (site, expansion) jobs"; return PCR_ERR_CAPACITY; }
		const uint32_t n_jobs = (uint32_t)n_jobs64;
		if((rc = ensure_dg_table(ctx, args->salt)) != PCR_OK) return rc;
		if(!ctx->site_attr_set){                                                   // (k_site_tm's own flag: the attribute is the kernel's)
			HIP_TRY(hipFuncSetAttribute((const void *)k_site_tm, hipFuncAttributeMaxDynamicSharedMemorySize, (int)SITE_LDS));
			ctx->site_attr_set = true;
		}
		if((rc = ctx->ptm_res.ensure(n_jobs)) != PCR_OK) return rc;
		if((rc = ctx->ptm_item_tm.ensure(ni)) != PCR_OK) return rc;
		// at most one block per CU (a block takes most of a CU's LDS), the waves striding over the jobs
		const unsigned grid_j = std::max(1u, std::min<unsigned>((n_jobs + SITE_WAVES - 1)/SITE_WAVES, (unsigned)ctx->n_cu));
		hipLaunchKernelGGL(k_site_tm, dim3(grid_j), dim3(SITE_THREADS), SITE_LDS, ctx->stream, S.db.p, S.db_cap, S.touched.p, S.d_seg_hi,
			(const uint2 *)ctx->ptm_items.p, ni, (const uint64_t *)ctx->ptm_joff.p, n_jobs, d_ol, d_olx, (const int *)ctx->th_dg.p, logf(args->salt), ctx->ptm_res.p);
		HIP_TRY(hipGetLastError());
		// ---- 3. Tm per item
		hipLaunchKernelGGL(k_item_tm, dim3(grid_i), dim3(POOL_THREADS), 0, ctx->stream, (const uint64_t *)ctx->ptm_joff.p, ni,
			(const float4 *)ctx->ptm_res.p, (ItemTm *)ctx->ptm_item_tm.p, ctx->ptm_flag.p);
		HIP_TRY(hipGetLastError());
		d_item_tm = (const ItemTm *)ctx->ptm_item_tm.p;                         // (the handle keeps it as uint2: the struct is this file's)
	}
	// ---- 4. the join: count (and the bits), scan
	unsigned long long *d_bits = nullptr;
	if(want_bits){
		if((rc = ctx->ptm_bits.ensure(2*row_words)) != PCR_OK) return rc;
		HIP_TRY(hipMemsetAsync(ctx->ptm_bits.p, 0, 2*row_words*sizeof(uint64_t), ctx->stream));
		d_bits = (unsigned long long *)ctx->ptm_bits.p;
	}
	if((rc = ctx->ptm_ioff.ensure((size_t)ni + 1)) != PCR_OK) return rc;
	HIP_TRY(hipMemsetAsync(ctx->ptm_cnt.p + ni, 0, sizeof(uint32_t), ctx->stream));
	hipLaunchKernelGGL(k_products_join<false>, dim3(grid_i), dim3(POOL_THREADS), 0, ctx->stream, S.db.p, S.db_cap, S.touched.p, S.d_seg_hi,
		ctx->ptm_items.p, ni, (const uint64_t *)ctx->ptm_eoff.p, d_ol, n_ol, S.planes.p, S.d_blk_off.p, S.d_len.p, S.d_has_eos.p,
		amp_min, amp_max, d_item_tm, tm_floor, d_intended, d_tab, (uint32_t)tab.size(), d_bits, n_pool, words,
		ctx->ptm_cnt.p, (const uint64_t *)nullptr, (pcr_product_tm *)nullptr, (uint64_t *)nullptr, (uint32_t *)nullptr);
	HIP_TRY(hipGetLastError());
	tmp = 0;
	HIP_TRY(rocprim::exclusive_scan(nullptr, tmp, ctx->ptm_cnt.p, ctx->ptm_ioff.p, uint64_t(0), (size_t)ni + 1, rocprim::plus<uint64_t>(), ctx->stream));
	if((rc = ctx->ptm_tmp.ensure(tmp + 16)) != PCR_OK) return rc;
	HIP_TRY(rocprim::exclusive_scan(ctx->ptm_tmp.p, tmp, ctx->ptm_cnt.p, ctx->ptm_ioff.p, uint64_t(0), (size_t)ni + 1, rocprim::plus<uint64_t>(), ctx->stream));
	uint64_t total = 0;
	uint32_t bad = 0;
	HIP_TRY(hipMemcpyAsync(&total, ctx->ptm_ioff.p + ni, sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
	HIP_TRY(hipMemcpyAsync(&bad, ctx->ptm_flag.p, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
	if(bits_fr) HIP_TRY(hipMemcpyAsync(bits_fr, ctx->ptm_bits.p, row_words*sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
	if(bits_rf) HIP_TRY(hipMemcpyAsync(bits_rf, ctx->ptm_bits.p + row_words, row_words*sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
	HIP_TRY(hipStreamSynchronize(ctx->stream));
	if(bad & 1u){ g_err = "pcr_pool_products_tm: internal trace-back error"; return PCR_ERR_RANGE; }
	// a pool pair that repeats an earlier one has that pair's rows (the device filled the first copy only)
	for(uint32_t i = 0;i < n_pool && want_bits;++i){
		const uint32_t f = oligo_id[2*i], r = oligo_id[2*i + 1];
		const uint32_t fr_first = tab_of[f*n_ol + r].fr_row, rf_first = tab_of[r*n_ol + f].rf_row;
		if(bits_fr && fr_first != i) memcpy(bits_fr + (size_t)i*words, bits_fr + (size_t)fr_first*words, words*sizeof(uint64_t));
		if(bits_rf && rf_first != i) memcpy(bits_rf + (size_t)i*words, bits_rf + (size_t)rf_first*words, words*sizeof(uint64_t));
	}
	if(total >= POOL_MAX_ITEMS){ g_err = "pcr_pool_products_tm: too many products"; return PCR_ERR_CAPACITY; }
	if(total == 0 || total > cap) return (int64_t)total;                         // count only: out is left as it is
	// ---- 4'. emit at the scanned offsets; 5. the key order
	const uint32_t nr = (uint32_t)total;
	if((rc = ctx->ptm_rec.ensure(2*(size_t)nr)) != PCR_OK) return rc;
	if((rc = ctx->ptm_keys.ensure(2*(size_t)nr)) != PCR_OK) return rc;
	if((rc = ctx->ptm_ord.ensure(2*(size_t)nr)) != PCR_OK) return rc;
	pcr_product_tm *r0 = ctx->ptm_rec.p, *r1 = r0 + nr;
	uint64_t *k0 = ctx->ptm_keys.p, *k1 = k0 + nr;
	uint32_t *o0 = ctx->ptm_ord.p, *o1 = o0 + nr;
	hipLaunchKernelGGL(k_products_join<true>, dim3(grid_i), dim3(POOL_THREADS), 0, ctx->stream, S.db.p, S.db_cap, S.touched.p, S.d_seg_hi,
		ctx->ptm_items.p, ni, (const uint64_t *)ctx->ptm_eoff.p, d_ol, n_ol, S.planes.p, S.d_blk_off.p, S.d_len.p, S.d_has_eos.p,
		amp_min, amp_max, d_item_tm, tm_floor, d_intended, d_tab, (uint32_t)tab.size(), (unsigned long long *)nullptr, n_pool, words,
		(uint32_t *)nullptr, (const uint64_t *)ctx->ptm_ioff.p, r0, k0, o0);
	HIP_TRY(hipGetLastError());
	const unsigned seq_bits = pool_bits(S.n), oligo_bits = pool_bits(n_ol);
	size_t t1 = 0, t2 = 0;
	HIP_TRY(rocprim::radix_sort_pairs(nullptr, t1, k0, k1, o0, o1, nr, 0, 64, ctx->stream));
	HIP_TRY(rocprim::radix_sort_pairs(nullptr, t2, k0, k1, o1, o0, nr, 0, 2*oligo_bits + seq_bits, ctx->stream));
	if((rc = ctx->ptm_tmp.ensure(std::max(t1, t2) + 16)) != PCR_OK) return rc;
	HIP_TRY(rocprim::radix_sort_pairs(ctx->ptm_tmp.p, t1, k0, k1, o0, o1, nr, 0, 64, ctx->stream));
	const unsigned grid_r = (nr + 255)/256;
	hipLaunchKernelGGL(k_products_key2, dim3(grid_r), dim3(256), 0, ctx->stream, (const pcr_product_tm *)r0, (const uint32_t *)o1, nr, seq_bits, oligo_bits, k0);
	HIP_TRY(hipGetLastError());
	HIP_TRY(rocprim::radix_sort_pairs(ctx->ptm_tmp.p, t2, k0, k1, o1, o0, nr, 0, 2*oligo_bits + seq_bits, ctx->stream));   // (stable)
	hipLaunchKernelGGL(k_products_gather, dim3(grid_r), dim3(256), 0, ctx->stream, (const pcr_product_tm *)r0, (const uint32_t *)o0, nr, d_intended, n_ol, r1);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipMemcpyAsync(out, r1, (size_t)nr*sizeof(pcr_product_tm), hipMemcpyDeviceToHost, ctx->stream));
	HIP_TRY(hipStreamSynchronize(ctx->stream));
	return (int64_t)total;
}

} // extern "C"
