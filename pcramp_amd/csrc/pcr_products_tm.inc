// Products of a primer pool with the Tm of their two sites, Tm-floored, and the pool's amplification bitsets at that floor
// (pcr_pool_products_tm; included by pcr_device.hip after pcr_pool.inc and pcr_site_tm.inc, whose stages it runs).
//
// pcr_pool_products and pcr_site_tm enumerate the same (entry, oligo) items with the same kernel, and k_pool_join forms a product
// from two item indices: with the site's tm_max stored per ITEM, a product's two Tm are two array reads and no lookup is made.
//   1. item_count / item_fill (pcr_pool.inc): the items and item_off.
//   2. melt_items (pcr_site_tm.inc): k_site_jobs + a scan, k_site_tm, one wave per (item, expansion) -> res[job].
//   3. Its k_item_tm: a thread per item walks its expansions in index order (strict >: the lowest index wins, no float atomics) ->
//      item_tm[k] = {tm_max, NO_TM}.  Indexed by item; the sites are never sorted.
//   4. k_products_join<false> / <true>: k_pool_join's walk (join_walk, pcr_pool.inc), plus the floor on
//      min(item_tm[k], item_tm[t]).  The count pass also sets the bits: a kept product whose (plus, minus) is a pool pair in
//      either orientation ORs bit `sequence` into that pair's row with a 64-bit atomicOr (many threads set the same bit and the
//      same word: the atomic is what makes that exact).  The emit pass writes the 48-byte records and their (begin, end) keys.
//   5. The record order: product_order (pcr_pool.inc), as pcr_pool_products.
// With tm_floor <= 0, cap = 0 and no bitset, steps 2 and 3 are skipped and the join only counts: pcr_pool_products' count.
// The items, jobs and Tm live in the scratch set this call shares with pcr_pool_probe_hits, pcr_pool_anneal_profile and
// pcr_pool_conflicts (pcr_ctx::shared: nothing in it outlives a call); the join's own buffers are pcr_ctx::ptm_*; the dG table is the handle's (th_dg, keyed by its salt as for every thermo call).

namespace {

struct ProductPair { uint32_t key, fr_row, rf_row, pad; };                      // key = plus*n_ol + minus -> the rows of the first pool pair (F, R) / (R, F) that it is
constexpr uint32_t PTM_NO_ROW = 0xFFFFFFFFu;

// What the join's bits need of a pool: the intended bitmap over (plus*n_ol + minus), and (plus, minus) -> the rows of the first pool
// pair that is (F, R) = (plus, minus) / (R, F) = (plus, minus), in key order (tab: what the device bisects).  Host side only;
// pcr_pool_products_end3 builds the same table.
struct PairTable {
	uint32_t n_ol;
	std::vector<uint32_t> intended;
	std::map<uint32_t, ProductPair> of;
	std::vector<ProductPair> tab;
	PairTable(const uint32_t *oligo_id, uint32_t n_pool, uint32_t n_oligos) : n_ol(n_oligos), intended(((size_t)n_oligos*n_oligos + 31)/32, 0)
	{
		for(uint32_t i = 0;i < n_pool;++i){
			const uint32_t f = oligo_id[2*i], r = oligo_id[2*i + 1];
			for(uint32_t b : {f*n_ol + r, r*n_ol + f}) intended[b >> 5] |= 1u << (b & 31);
			for(int o = 0;o < 2;++o){
				const uint32_t b = o ? r*n_ol + f : f*n_ol + r;
				ProductPair fresh; fresh.key = b; fresh.fr_row = fresh.rf_row = PTM_NO_ROW; fresh.pad = 0;
				ProductPair &pp = of.insert(std::make_pair(b, fresh)).first->second;
				uint32_t &row = o ? pp.rf_row : pp.fr_row;
				if(row == PTM_NO_ROW) row = i;
			}
		}
		tab.reserve(of.size());
		for(const auto &kv : of) tab.push_back(kv.second);                       // (key order)
	}
	// a pool pair that repeats an earlier one has that pair's rows (the device filled the first copy only)
	void copy_repeated_rows(const uint32_t *oligo_id, uint32_t n_pool, uint32_t words, uint64_t *bits_fr, uint64_t *bits_rf)
	{
		for(uint32_t i = 0;i < n_pool && (bits_fr || bits_rf);++i){
			const uint32_t f = oligo_id[2*i], r = oligo_id[2*i + 1];
			const uint32_t fr_first = of[f*n_ol + r].fr_row, rf_first = of[r*n_ol + f].rf_row;
			if(bits_fr && fr_first != i) memcpy(bits_fr + (size_t)i*words, bits_fr + (size_t)fr_first*words, words*sizeof(uint64_t));
			if(bits_rf && rf_first != i) memcpy(bits_rf + (size_t)i*words, bits_rf + (size_t)rf_first*words, words*sizeof(uint64_t));
		}
	}
};

// k_pool_join with the two sites' Tm: one thread per item k, join_walk.  item_tm = NULL: no Tm is read and nothing is floored (the
// plain count).  <false>: count[k], and with bits != NULL the bit of every kept product of a pool pair; <true>: records, (begin, end)
// sort keys and identity indices at rec_off[k] ..
template<bool EMIT>
__global__ __launch_bounds__(POOL_THREADS) void k_products_join(const JoinIn J, const ItemTm *__restrict__ item_tm, float tm_floor,
	const uint32_t *__restrict__ intended, const ProductPair *__restrict__ pair_tab, uint32_t n_tab, unsigned long long *__restrict__ bits,
	uint32_t n_pool, uint32_t words, uint32_t *__restrict__ count, const uint64_t *__restrict__ rec_off, pcr_product_tm *__restrict__ rec,
	uint64_t *__restrict__ key, uint32_t *__restrict__ ord)
{
	__shared__ int2 ss[POOL_MAX_OLIGOS];
	join_geometry(J, ss);
	const uint32_t k = blockIdx.x*blockDim.x + threadIdx.x;
	if(k >= J.n_items) return;
	const uint2 it = J.items[k];
	const uint32_t g = it.x, x = it.y;
	const uint32_t i = J.touched[g/J.cap]*J.cap + g % J.cap;
	const DevEntry ei = J.db[i];
	uint32_t c = 0;
	uint64_t w = EMIT ? rec_off[k] : 0;
	if(ei.strand == 1){
		ItemTm tp; tp.tm = 0.0f; tp.no_tm = 0;
		if(item_tm) tp = item_tm[k];
		const bool floored = item_tm && tm_floor > 0.0f;
		auto keep = [&](uint64_t t, uint32_t y, uint32_t, int32_t p5, int32_t m3, int32_t in_start, int32_t in_len){
			ItemTm tm; tm.tm = 0.0f; tm.no_tm = 0;
			if(item_tm) tm = item_tm[t];
			if(floored && !(((tp.tm < tm.tm) ? tp.tm : tm.tm) >= tm_floor)) return;   // min(tm_plus, tm_minus) >= tm_floor
			if(EMIT){
				pcr_product_tm r;
				r.plus_oligo = x; r.minus_oligo = y; r.sequence = ei.seq; r.begin = p5; r.end = m3;
				r.inner_start = in_start; r.inner_length = in_len; r.intended = 0;
				r.tm_plus = tp.tm; r.tm_minus = tm.tm;
				r.flags = (tp.no_tm ? PCR_PRODUCT_PLUS_NO_TM : 0u) | (tm.no_tm ? PCR_PRODUCT_MINUS_NO_TM : 0u);
				r.reserved = 0;
				rec[w] = r;
				key[w] = product_key1(p5, m3);
				ord[w] = (uint32_t)w;
				++w;
			}
			else{
				++c;
				const uint32_t b = x*J.n_ol + y;
				if(bits && ((intended[b >> 5] >> (b & 31)) & 1u)){
					uint32_t lo = 0, above = n_tab;                                  // pair_tab[lo].key <= b < pair_tab[above].key; an intended b is in the table
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
		};
		if(!(floored && tp.tm < tm_floor)) join_walk<false>(J, ss, g, x, i, ei, 0u, keep);   // (a plus site below the floor keeps no product)
	}
	if(!EMIT) count[k] = c;
}

} // namespace

extern "C" {

int64_t pcr_pool_products_tm(pcr_ctx *ctx, pcr_set which, const pcr_pair *pool, uint32_t n_pool, float threshold,
	int32_t amp_min, int32_t amp_max, const pcr_thermo_args *args, float template_strand, float tm_floor,
	uint32_t *oligo_id, pcr_product_tm *out, uint64_t cap, uint64_t *bits_fr, uint64_t *bits_rf)
{
	static_assert(sizeof(pcr_product_tm) == 48, "record layout");
	static_assert(sizeof(ProductPair) == 16, "table layout");
	static_assert((uint64_t)POOL_MAX_OLIGOS*POOL_MAX_OLIGOS <= 0xFFFFFFFFull, "a (plus, minus) key is 32-bit");
	// ---- the arguments, before the handle (pcr_site_tm's checks in its order, the oligo table, then the floor)
	if(!set_ok(which)){ g_err = "pcr_pool_products_tm: unknown sequence set"; return PCR_ERR_ARG; }
	if(which != PCR_SET_TARGET && which != PCR_SET_BACKGROUND){ g_err = "pcr_pool_products_tm: PCR_SET_MULTIPLEX is not supported (PCR_SET_TARGET or PCR_SET_BACKGROUND)"; return PCR_ERR_ARG; }
	if(!args || (n_pool && (!pool || !oligo_id)) || (cap && !out)){ g_err = "pcr_pool_products_tm: bad argument"; return PCR_ERR_ARG; }
	if(n_pool > PCR_POOL_MAX_PAIRS){ g_err = "pcr_pool_products_tm: pool larger than PCR_POOL_MAX_PAIRS"; return PCR_ERR_ARG; }
	if(!(template_strand >= 0.0f) || !(args->primer_strand >= 0.0f)){ g_err = "pcr_pool_products_tm: negative strand concentration (NucCruc::strand, nuc_cruc.h:818-826)"; return PCR_ERR_ARG; }
	if(!(args->salt >= 1.0e-6f && args->salt <= 1.0f)){ g_err = "pcr_pool_products_tm: salt outside [1e-6, 1] (NucCruc::salt, nuc_cruc.h:780-788)"; return PCR_ERR_ARG; }
	std::vector<PoolOligo> ol;
	std::vector<SiteOligoX> olx;
	if(site_oligo_table("pcr_pool_products_tm", "an oligo", "primer_strand", pool, n_pool, threshold, args, template_strand, oligo_id, ol, olx) != PCR_OK) return PCR_ERR_ARG;
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
	PairTable pair_rows(oligo_id, n_pool, n_ol);
	const std::vector<uint32_t> &intended = pair_rows.intended;
	const std::vector<ProductPair> &tab = pair_rows.tab;
	int rc;
	const size_t ol_bytes = ol.size()*sizeof(PoolOligo), tab_bytes = tab.size()*sizeof(ProductPair), olx_bytes = olx.size()*sizeof(SiteOligoX),
		int_bytes = intended.size()*sizeof(uint32_t);
	std::vector<uint8_t> blob(ol_bytes + tab_bytes + olx_bytes + int_bytes);     // 32-, 16-, 8- and 4-byte records, in that order: each is aligned
	memcpy(blob.data(), ol.data(), ol_bytes);
	memcpy(blob.data() + ol_bytes, tab.data(), tab_bytes);
	memcpy(blob.data() + ol_bytes + tab_bytes, olx.data(), olx_bytes);
	memcpy(blob.data() + ol_bytes + tab_bytes + olx_bytes, intended.data(), int_bytes);
	ItemScratch &X = ctx->shared;
	const ItemBufs B = X.bufs();
	if((rc = X.in.ensure(blob.size())) != PCR_OK) return rc;
	const PoolOligo *d_ol = (const PoolOligo *)X.in.p;
	const ProductPair *d_tab = (const ProductPair *)(X.in.p + ol_bytes);
	const SiteOligoX *d_olx = (const SiteOligoX *)(X.in.p + ol_bytes + tab_bytes);
	const uint32_t *d_intended = (const uint32_t *)(X.in.p + ol_bytes + tab_bytes + olx_bytes);
	HIP_TRY(hipMemcpyAsync(X.in.p, blob.data(), blob.size(), hipMemcpyHostToDevice, ctx->stream));
	// ---- 1. the items (item_count waits: blob is read by then)
	uint64_t n_items = 0;
	if((rc = item_count(ctx, S, d_ol, n_ol, B, n_items)) != PCR_OK) return rc;
	if(n_items >= POOL_MAX_ITEMS){ g_err = "pcr_pool_products_tm: too many (entry, oligo) hits"; return PCR_ERR_CAPACITY; }
	if(n_items == 0){ zero_rows(); return 0; }
	if((rc = item_fill(ctx, S, d_ol, n_ol, B, n_items)) != PCR_OK) return rc;
	const uint32_t ni = (uint32_t)n_items;
	const unsigned grid_i = (ni + POOL_THREADS - 1)/POOL_THREADS;
	if((rc = X.cnt.ensure((size_t)ni + 1)) != PCR_OK) return rc;                // (the entry counts are spent)
	// ---- 2. job offsets, the jobs; 3. Tm per item
	if(melt && (rc = melt_items("pcr_pool_products_tm", ctx, S, d_ol, d_olx, ni, args->salt, B)) != PCR_OK) return rc;
	const ItemTm *d_item_tm = melt ? (const ItemTm *)X.item_tm.p : nullptr;
	// ---- 4. the join: count (and the bits), scan
	unsigned long long *d_bits = nullptr;
	if(want_bits){
		if((rc = ctx->ptm_bits.ensure(2*row_words)) != PCR_OK) return rc;
		HIP_TRY(hipMemsetAsync(ctx->ptm_bits.p, 0, 2*row_words*sizeof(uint64_t), ctx->stream));
		d_bits = (unsigned long long *)ctx->ptm_bits.p;
	}
	const JoinIn J{S.db.p, S.db_cap, S.touched.p, S.d_seg_hi, X.items.p, ni, X.eoff.p, d_ol, n_ol, S.planes.p, S.d_blk_off.p, S.d_len.p,
		S.d_has_eos.p, amp_min, amp_max};
	hipLaunchKernelGGL(k_products_join<false>, dim3(grid_i), dim3(POOL_THREADS), 0, ctx->stream, J, d_item_tm, tm_floor, d_intended, d_tab,
		(uint32_t)tab.size(), d_bits, n_pool, words, X.cnt.p, (const uint64_t *)nullptr, (pcr_product_tm *)nullptr, (uint64_t *)nullptr, (uint32_t *)nullptr);
	HIP_TRY(hipGetLastError());
	uint64_t total = 0;
	uint32_t bad = 0;                                                            // (without a melt no k_item_tm ran: the flag is another call's)
	if((rc = scan_total(ctx, X.cnt.p, X.ioff, X.tmp, ni, total, [&]() -> int {
		if(melt) HIP_TRY(hipMemcpyAsync(&bad, X.flag.p, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
		if(bits_fr) HIP_TRY(hipMemcpyAsync(bits_fr, ctx->ptm_bits.p, row_words*sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
		if(bits_rf) HIP_TRY(hipMemcpyAsync(bits_rf, ctx->ptm_bits.p + row_words, row_words*sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
		return PCR_OK;
	})) != PCR_OK) return rc;
	if(bad & 1u){ g_err = "pcr_pool_products_tm: internal trace-back error"; return PCR_ERR_RANGE; }
	pair_rows.copy_repeated_rows(oligo_id, n_pool, words, bits_fr, bits_rf);
	if(total >= POOL_MAX_ITEMS){ g_err = "pcr_pool_products_tm: too many products"; return PCR_ERR_CAPACITY; }
	if(total == 0 || total > cap) return (int64_t)total;                         // count only: out is left as it is
	// ---- 4'. emit at the scanned offsets; 5. the key order
	const uint32_t nr = (uint32_t)total;
	if((rc = ctx->ptm_rec.ensure(2*(size_t)nr)) != PCR_OK) return rc;
	if((rc = ctx->ptm_keys.ensure(2*(size_t)nr)) != PCR_OK) return rc;
	if((rc = ctx->ptm_ord.ensure(2*(size_t)nr)) != PCR_OK) return rc;
	pcr_product_tm *r0 = ctx->ptm_rec.p, *r1 = r0 + nr;
	hipLaunchKernelGGL(k_products_join<true>, dim3(grid_i), dim3(POOL_THREADS), 0, ctx->stream, J, d_item_tm, tm_floor, d_intended, d_tab,
		(uint32_t)tab.size(), (unsigned long long *)nullptr, n_pool, words, (uint32_t *)nullptr, (const uint64_t *)X.ioff.p, r0, ctx->ptm_keys.p, ctx->ptm_ord.p);
	HIP_TRY(hipGetLastError());
	if((rc = product_order(ctx, r0, ctx->ptm_keys.p, ctx->ptm_ord.p, nr, pool_bits(S.n), pool_bits(n_ol), d_intended, n_ol, X.tmp)) != PCR_OK) return rc;
	HIP_TRY(hipMemcpyAsync(out, r1, (size_t)nr*sizeof(pcr_product_tm), hipMemcpyDeviceToHost, ctx->stream));
	HIP_TRY(hipStreamSynchronize(ctx->stream));
	return (int64_t)total;
}

} // extern "C"
