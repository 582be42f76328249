// Which products of a pool a probe binds inside, and which sequences each (F, R, probe) assay detects (pcr_pool_probe_hits;
// included by pcr_device.hip after pcr_pool.inc and pcr_site_tm.inc, whose item and melt stages it runs).
//
// One oligo table holds the pool's distinct primers (pcr_pool_products' ids 0 .. n_prim - 1) and then its distinct probes
// (table entry n_prim + probe id); SiteOligoX::log_strand carries each oligo's own concentration.  The (entry, oligo) items,
// their jobs and item_tm[] are then pcr_pool_products_tm's steps 1-3 over that table (item_count / item_fill, melt_items).
// From there:
//   4. k_probe_products<false> / <true>: k_products_join's walk (join_walk) and floor, with primer items only in either role.
//      The count pass also ORs the bit of every kept product of a pool pair WITHOUT a probe into that pair's row (its row is
//      pcr_pool_products_tm's fr | rf); the emit pass compacts the kept products: {plus item, minus item, plus slot, minus slot}.
//   5. k_probe_hits<false> / <true>: one wave per kept product.  A probe site inside it (p3 < loc5, loc3 < m5) lies on an entry
//      with p3 - 31 < loc < m5 + 31, whichever slots the three oligos occupy in their words; the entries of a segment are sorted
//      by loc and the items are a CSR over the entries, so those entries' items are ONE contiguous run, found by two bisections.
//      The lanes stride over the run and test the items that are probes: a product with a dense bucket between its primers costs
//      its wave more steps, not one thread a cubic loop.  The count pass ORs the bit of every hit of an intended (plus, minus,
//      probe) into that assay's row; the emit pass places each hit by a ballot prefix at the scanned offset (no atomics: where a
//      record lands does not depend on scheduling).
//   6. The record order: three stable radix sorts, least significant key first -- (probe, probe_loc5, probe_strand), (begin, end),
//      (plus_oligo, minus_oligo, sequence) -- and a gather.
// pcr_pool_probe_hits_end3 is the same call with a 3'-end rule (pcr_products_end3.inc, included before this file) in step 4:
// k_item_end3 fills an ItemEnd per item before the melt (the probes' too; nobody reads them), and k_probe_products' functor makes
// k_end3_join's tests behind the floor.  Step 5 sees fewer products and is what it was.
// Steps 1-3 work in the scratch set shared with pcr_pool_products_tm and the others (pcr_ctx::shared), the rest in pcr_ctx::pph_*; the dG table is the handle's (th_dg, keyed by its salt as for every thermo call).

namespace {

struct ProbeAssay { uint64_t key; uint32_t row, pad; };                        // key = (plus*n_prim + minus) << 32 | probe (PCR_NO_PROBE: none) -> the first pool pair that is it, in either orientation
constexpr int PPH_WAVES = 4;                                                    // waves per block of k_probe_hits
constexpr uint32_t PPH_NO_ROW = 0xFFFFFFFFu;

// tab[lo].key <= key < tab[above].key -> the row, or PPH_NO_ROW
__device__ __forceinline__ uint32_t probe_assay_row(const ProbeAssay *__restrict__ tab, uint32_t n_tab, uint64_t key)
{
	if(n_tab == 0) return PPH_NO_ROW;
	uint32_t lo = 0, above = n_tab;
	while(above - lo > 1u){
		const uint32_t mid = lo + (above - lo)/2u;
		if(tab[mid].key <= key) lo = mid; else above = mid;
	}
	const ProbeAssay a = tab[lo];
	return (a.key == key) ? a.row : PPH_NO_ROW;
}

// k_products_join over the primer items (oligo < n_prim) of a table that also lists probes: join_walk<true> with n_minus = n_prim.
// <false>: count[k], and with bits != NULL the bit of every kept product whose (plus, minus) is a pool pair without a probe;
// <true>: the kept products at prod_off[k] .. as {k, t, plus slot, minus slot}.  item_end != NULL: a kept product also passes the
// 3'-end rule R on its two primer sites (k_end3_join's tests, after the floor); a probe's ItemEnd is never read.
template<bool EMIT>
__global__ __launch_bounds__(POOL_THREADS) void k_probe_products(const JoinIn J, uint32_t n_prim, const ItemTm *__restrict__ item_tm, float tm_floor,
	const ItemEnd *__restrict__ item_end, const End3Rule R, const uint32_t *__restrict__ intended, const ProbeAssay *__restrict__ tab, uint32_t n_tab, unsigned long long *__restrict__ bits, uint32_t words,
	uint32_t *__restrict__ count, const uint64_t *__restrict__ prod_off, uint4 *__restrict__ prod)
{
	__shared__ int2 ss[POOL_MAX_OLIGOS];
	join_geometry(J, ss);
	const uint32_t k = blockIdx.x*blockDim.x + threadIdx.x;
	if(k >= J.n_items) return;
	const uint2 it = J.items[k];
	const uint32_t g = it.x, x = it.y;
	uint32_t c = 0;
	uint64_t w = EMIT ? prod_off[k] : 0;
	if(x < n_prim){                                                             // (a probe takes no primer role)
		const uint32_t i = J.touched[g/J.cap]*J.cap + g % J.cap;
		const DevEntry ei = J.db[i];
		if(ei.strand == 1){
			const ItemTm tp = item_tm[k];
			const bool floored = tm_floor > 0.0f;
			ItemEnd ep; ep.clamp3 = ep.end_mismatch = ep.length = ep.pad = 0; ep.id = 0.0f;
			if(item_end) ep = item_end[k];
			const bool plus_ok = !item_end || end3_site_ok(ep, R);
			auto keep = [&](uint64_t t, uint32_t y, uint32_t j, int32_t, int32_t, int32_t, int32_t){
				const ItemTm tm = item_tm[t];
				if(floored && !(((tp.tm < tm.tm) ? tp.tm : tm.tm) >= tm_floor)) return;   // min(tm_plus, tm_minus) >= tm_floor
				ItemEnd em;
				if(item_end && !end3_product_ok(item_end, R, plus_ok, ep, t, em)) return;
				if(EMIT) prod[w++] = make_uint4(k, (uint32_t)t, i, j);
				else{
					++c;
					const uint32_t b = x*n_prim + y;
					if(bits && ((intended[b >> 5] >> (b & 31)) & 1u)){
						const uint32_t row = probe_assay_row(tab, n_tab, ((uint64_t)b << 32) | PCR_NO_PROBE);
						if(row != PPH_NO_ROW) atomicOr(bits + (size_t)row*words + (ei.seq >> 6), 1ull << (ei.seq & 63u));
					}
				}
			};
			// (a plus site below the floor keeps no product, nor does one that fails its own half of the rule)
			if(!(floored && tp.tm < tm_floor) && plus_ok) join_walk<true>(J, ss, g, x, i, ei, n_prim, keep);
		}
	}
	if(!EMIT) count[k] = c;
}

// first slot of [lo, hi) whose loc >= v (the entries of a segment are sorted by loc)
__device__ __forceinline__ uint32_t probe_lower_bound(const DevEntry *__restrict__ db, uint32_t lo, uint32_t hi, int32_t v)
{
	while(lo < hi){
		const uint32_t mid = lo + (hi - lo)/2u;
		if(db[mid].loc < v) lo = mid + 1u; else hi = mid;
	}
	return lo;
}

// One wave per kept product p = {k, t, i, j}: the probe items on the entries with p3 - 31 < loc < m5 + 31 of its segment.
// <false>: count[p], and with bits != NULL the bit of every hit whose (plus, minus, probe) is an assay of the pool;
// <true>: the records, their first sort key and identity indices at rec_off[p] ..
template<bool EMIT>
__global__ __launch_bounds__(64*PPH_WAVES) void k_probe_hits(const DevEntry *__restrict__ db, uint32_t cap, const uint32_t *__restrict__ seg_hi,
	const uint2 *__restrict__ items, const uint64_t *__restrict__ item_off, const PoolOligo *__restrict__ oligos, uint32_t n_ol, uint32_t n_prim,
	const uint4 *__restrict__ prod, uint32_t n_prod, const ItemTm *__restrict__ item_tm, float probe_tm_floor,
	const uint32_t *__restrict__ intended, const ProbeAssay *__restrict__ tab, uint32_t n_tab, unsigned long long *__restrict__ bits, uint32_t words,
	uint32_t *__restrict__ count, const uint64_t *__restrict__ rec_off, pcr_probe_hit *__restrict__ rec, uint64_t *__restrict__ key,
	uint32_t *__restrict__ ord)
{
	__shared__ int2 ss[POOL_MAX_OLIGOS];                                        // Word::start() / stop()
	for(uint32_t o = threadIdx.x;o < n_ol;o += blockDim.x) ss[o] = make_int2(oligos[o].start, oligos[o].stop);
	__syncthreads();
	const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63u;   // (uniform: the product's loads and both bisections run once per wave)
	const unsigned long long below = (1ull << lane) - 1ull;
	for(uint32_t p = blockIdx.x*PPH_WAVES + wave;p < n_prod;p += gridDim.x*PPH_WAVES){   // uniform per wave
		const uint4 pr = prod[p];
		const uint2 ik = items[pr.x], itm = items[pr.y];
		const uint32_t x = ik.y, y = itm.y;
		const DevEntry ei = db[pr.z], ej = db[pr.w];
		const int2 P = ss[x], M = ss[y];
		const int32_t p5 = ei.loc + P.x, p3 = ei.loc + P.y, m5 = ej.loc - M.y, m3 = ej.loc - M.x;
		const uint32_t seg_lo = ei.seq*cap, hi = seg_hi[ei.seq];
		// slots e_lo .. e_hi - 1: p3 - 31 < loc < m5 + 31; their items are item_off[g(e_lo)] .. item_off[g(e_hi)] - 1
		const uint32_t e_lo = probe_lower_bound(db, seg_lo, hi, p3 - 30), e_hi = probe_lower_bound(db, e_lo, hi, m5 + 31);
		const uint32_t g0 = ik.x - (pr.z - seg_lo);                               // DB thread of the segment's first slot
		const uint64_t t_lo = item_off[g0 + (e_lo - seg_lo)], t_hi = item_off[g0 + (e_hi - seg_lo)];
		const uint32_t b = x*n_prim + y;
		uint32_t c = 0;
		uint64_t w = EMIT ? rec_off[p] : 0;
		for(uint64_t base = t_lo;base < t_hi;base += 64){                         // (uniform trip count: the ballots below are the whole wave's)
			const uint64_t t = base + lane;
			bool hit = false;
			uint32_t q = 0, strand = 0;
			int32_t loc5 = 0, loc3 = 0;
			ItemTm tq; tq.tm = 0.0f; tq.no_tm = 0;
			if(t < t_hi){
				const uint2 iq = items[t];
				if(iq.y >= n_prim){                                                // (a primer takes no probe role)
					q = iq.y - n_prim;
					const DevEntry e = db[seg_lo + (iq.x - g0)];
					const int2 Q = ss[iq.y];
					strand = e.strand;
					loc5 = (strand == 1) ? e.loc + Q.x : e.loc - Q.y;               // sequence.h:57-75
					loc3 = (strand == 1) ? e.loc + Q.y : e.loc - Q.x;
					if(p3 < loc5 && loc3 < m5){
						tq = item_tm[t];
						hit = !(probe_tm_floor > 0.0f) || tq.tm >= probe_tm_floor;
					}
				}
			}
			const unsigned long long mask = __ballot(hit);
			if(EMIT){
				if(hit){
					const uint64_t at = w + (uint64_t)__popcll(mask & below);
					const ItemTm tp = item_tm[pr.x], tm = item_tm[pr.y];
					pcr_probe_hit r;
					r.plus_oligo = x; r.minus_oligo = y; r.probe = q; r.sequence = ei.seq;
					r.begin = p5; r.end = m3; r.inner_start = p3 + 1 - 4; r.inner_length = m5 - r.inner_start + 8;
					r.probe_loc5 = loc5; r.probe_loc3 = loc3; r.probe_strand = strand;
					r.intended = (((intended[b >> 5] >> (b & 31)) & 1u) ? PCR_HIT_PRODUCT_INTENDED : 0u)
						| ((probe_assay_row(tab, n_tab, ((uint64_t)b << 32) | q) != PPH_NO_ROW) ? PCR_HIT_PROBE_INTENDED : 0u);
					r.tm_plus = tp.tm; r.tm_minus = tm.tm; r.tm_probe = tq.tm;
					r.flags = (tp.no_tm ? PCR_PRODUCT_PLUS_NO_TM : 0u) | (tm.no_tm ? PCR_PRODUCT_MINUS_NO_TM : 0u) | (tq.no_tm ? PCR_HIT_PROBE_NO_TM : 0u);
					rec[at] = r;
					key[at] = ((uint64_t)q << 33) | ((uint64_t)((uint32_t)loc5 ^ 0x80000000u) << 1) | (strand - 1u);   // signed order
					ord[at] = (uint32_t)at;
				}
				w += (uint64_t)__popcll(mask);
			}
			else{
				c += (uint32_t)__popcll(mask);
				if(hit && bits && ((intended[b >> 5] >> (b & 31)) & 1u)){
					const uint32_t row = probe_assay_row(tab, n_tab, ((uint64_t)b << 32) | q);
					if(row != PPH_NO_ROW) atomicOr(bits + (size_t)row*words + (ei.seq >> 6), 1ull << (ei.seq & 63u));
				}
			}
		}
		if(!EMIT && lane == 0) count[p] = c;
	}
}

// the next sort key of the records in their present order; stage 1: (begin, end), stage 2: (plus_oligo, minus_oligo, sequence)
__global__ void k_probe_key(const pcr_probe_hit *__restrict__ rec, const uint32_t *__restrict__ ord, uint32_t n, int stage, uint32_t seq_bits,
	uint32_t oligo_bits, uint64_t *__restrict__ key)
{
	const uint32_t r = blockIdx.x*blockDim.x + threadIdx.x;
	if(r >= n) return;
	const uint32_t at = ord[r];
	if(stage == 1) key[r] = ((uint64_t)((uint32_t)rec[at].begin ^ 0x80000000u) << 32) | ((uint32_t)rec[at].end ^ 0x80000000u);   // signed order
	else key[r] = ((uint64_t)rec[at].plus_oligo << (oligo_bits + seq_bits)) | ((uint64_t)rec[at].minus_oligo << seq_bits) | rec[at].sequence;
}

__global__ void k_probe_gather(const pcr_probe_hit *__restrict__ rec, const uint32_t *__restrict__ ord, uint32_t n, pcr_probe_hit *__restrict__ out)
{
	const uint32_t r = blockIdx.x*blockDim.x + threadIdx.x;
	if(r < n) out[r] = rec[ord[r]];
}

// pcr_pool_probe_hits (rule = NULL) and pcr_pool_probe_hits_end3; who: the entry point's name, for the refusals
int64_t probe_hits_impl(const std::string &who, pcr_ctx *ctx, pcr_set which, const pcr_pair *pool, const pcr_word128 *probes, uint32_t n_pool,
	float threshold, int32_t amp_min, int32_t amp_max, const pcr_thermo_args *args, float probe_strand_conc, float template_strand,
	float tm_floor, float probe_tm_floor, const pcr_end3_rule *rule, uint32_t *oligo_id, uint32_t *probe_id, pcr_probe_hit *out, uint64_t cap,
	uint64_t *detected)
{
	static_assert(sizeof(pcr_probe_hit) == 64, "record layout");
	static_assert(sizeof(ProbeAssay) == 16, "table layout");
	// ---- the arguments, before the handle (pcr_pool_products_tm's checks in its order, the probes after the primers)
	if(!set_ok(which)){ g_err = who + ": unknown sequence set"; return PCR_ERR_ARG; }
	if(which != PCR_SET_TARGET && which != PCR_SET_BACKGROUND){ g_err = who + ": PCR_SET_MULTIPLEX is not supported (PCR_SET_TARGET or PCR_SET_BACKGROUND)"; return PCR_ERR_ARG; }
	if(!args || (n_pool && (!pool || !probes || !oligo_id || !probe_id)) || (cap && !out)){ g_err = who + ": bad argument"; return PCR_ERR_ARG; }
	if(n_pool > PCR_POOL_MAX_PAIRS){ g_err = who + ": pool larger than PCR_POOL_MAX_PAIRS"; return PCR_ERR_ARG; }
	if(!(template_strand >= 0.0f) || !(args->primer_strand >= 0.0f) || !(probe_strand_conc >= 0.0f)){ g_err = who + ": negative strand concentration (NucCruc::strand, nuc_cruc.h:818-826)"; return PCR_ERR_ARG; }
	if(!(args->salt >= 1.0e-6f && args->salt <= 1.0f)){ g_err = who + ": salt outside [1e-6, 1] (NucCruc::salt, nuc_cruc.h:780-788)"; return PCR_ERR_ARG; }
	// the distinct primers in order of first appearance (as pcr_pool_products), then the distinct probes in theirs
	std::vector<PoolOligo> ol;
	std::vector<SiteOligoX> olx;
	const float thr2 = threshold*threshold;                                      // pcr_assay.cpp:775-776
	if(site_oligo_table(who, "a primer", "its concentration", pool, n_pool, threshold, args, template_strand, oligo_id, ol, olx) != PCR_OK) return PCR_ERR_ARG;
	const uint32_t n_prim = (uint32_t)ol.size();
	std::map<std::pair<uint64_t, uint64_t>, uint32_t> probe_of;
	for(uint32_t i = 0;i < n_pool;++i){
		const pcr_word128 &wd = probes[i];
		if(!wd.w[0] && !wd.w[1]){ probe_id[i] = PCR_NO_PROBE; continue; }
		auto ins = probe_of.insert(std::make_pair(std::make_pair(wd.w[0], wd.w[1]), (uint32_t)probe_of.size()));
		if(ins.second){
			PoolOligo p; SiteOligoX x;
			if(!site_oligo(who, "a probe", wd, thr2, true, probe_strand_conc, "its concentration", template_strand, p, x)) return PCR_ERR_ARG;
			ol.push_back(p); olx.push_back(x);
		}
		probe_id[i] = ins.first->second;
	}
	if(ol.size() > POOL_MAX_OLIGOS){ g_err = who + ": too many distinct oligos (primers plus probes over 2*PCR_POOL_MAX_PAIRS)"; return PCR_ERR_ARG; }
	if(!std::isfinite(tm_floor)){ g_err = who + ": tm_floor is not finite"; return PCR_ERR_ARG; }
	if(!std::isfinite(probe_tm_floor)){ g_err = who + ": probe_tm_floor is not finite"; return PCR_ERR_ARG; }
	End3Rule R;
	int use_taq;
	if(end3_rule_of(who, rule, R, use_taq) != PCR_OK) return PCR_ERR_ARG;
	const bool ruled = end3_ruled(R);                                            // else: no ItemEnd is computed, the join is the base call's
	if(!ctx){ g_err = who + ": null handle"; return PCR_ERR_ARG; }
	{ const int drc = drain(ctx); if(drc != PCR_OK) return drc; }
	HIP_TRY(hipSetDevice(ctx->device));
	SeqSet &S = ctx->sets[which];
	if(!S.have_db){ g_err = who + ": no word DB (call pcr_select_sites over the pool and its probes first)"; return PCR_ERR_STATE; }
	if(n_pool == 0) return 0;
	const uint32_t words = (uint32_t)((S.n + 63)/64);
	const size_t row_words = (size_t)n_pool*words;
	// whatever the count, the rows asked for are written in full
	auto zero_rows = [&](){ if(detected) memset(detected, 0, row_words*sizeof(uint64_t)); };
	{ const int erc = ensure_touched(ctx, S); if(erc != PCR_OK) return erc; }
	if(S.n_entries == 0 || S.n_touched == 0){ zero_rows(); return 0; }
	const uint32_t n_ol = (uint32_t)ol.size();
	// the intended bitmap over the primers, and (plus, minus, probe) -> the row of the first pool pair that is it in either orientation
	std::vector<uint32_t> intended(((size_t)n_prim*n_prim + 31)/32, 0);
	std::map<uint64_t, uint32_t> row_of;
	std::vector<uint32_t> first_row(n_pool);
	for(uint32_t i = 0;i < n_pool;++i){
		const uint32_t f = oligo_id[2*i], r = oligo_id[2*i + 1];
		for(uint32_t b : {f*n_prim + r, r*n_prim + f}){
			intended[b >> 5] |= 1u << (b & 31);
			first_row[i] = row_of.insert(std::make_pair(((uint64_t)b << 32) | probe_id[i], i)).first->second;   // (both orientations were inserted together: one row)
		}
	}
	std::vector<ProbeAssay> tab;
	tab.reserve(row_of.size());
	for(const auto &kv : row_of){ ProbeAssay a; a.key = kv.first; a.row = kv.second; a.pad = 0; tab.push_back(a); }   // (key order)
	int rc;
	const size_t ol_bytes = ol.size()*sizeof(PoolOligo), tab_bytes = tab.size()*sizeof(ProbeAssay), olx_bytes = olx.size()*sizeof(SiteOligoX),
		int_bytes = intended.size()*sizeof(uint32_t);
	const std::vector<float> norm = ruled ? end3_norms(ol) : std::vector<float>();   // (k_item_end3's, the probes included; only a rule reads it)
	const size_t norm_bytes = norm.size()*sizeof(float);
	std::vector<uint8_t> blob(ol_bytes + tab_bytes + olx_bytes + int_bytes + norm_bytes);   // 32-, 16-, 8-, 4- and 4-byte records, in that order: each is aligned
	memcpy(blob.data(), ol.data(), ol_bytes);
	memcpy(blob.data() + ol_bytes, tab.data(), tab_bytes);
	memcpy(blob.data() + ol_bytes + tab_bytes, olx.data(), olx_bytes);
	memcpy(blob.data() + ol_bytes + tab_bytes + olx_bytes, intended.data(), int_bytes);
	if(norm_bytes) memcpy(blob.data() + ol_bytes + tab_bytes + olx_bytes + int_bytes, norm.data(), norm_bytes);
	ItemScratch &X = ctx->shared;
	const ItemBufs B = X.bufs();
	if((rc = X.in.ensure(blob.size())) != PCR_OK) return rc;
	const PoolOligo *d_ol = (const PoolOligo *)X.in.p;
	const ProbeAssay *d_tab = (const ProbeAssay *)(X.in.p + ol_bytes);
	const SiteOligoX *d_olx = (const SiteOligoX *)(X.in.p + ol_bytes + tab_bytes);
	const uint32_t *d_intended = (const uint32_t *)(X.in.p + ol_bytes + tab_bytes + olx_bytes);
	const float *d_norm = (const float *)(X.in.p + ol_bytes + tab_bytes + olx_bytes + int_bytes);
	const uint32_t n_tab = (uint32_t)tab.size();
	HIP_TRY(hipMemcpyAsync(X.in.p, blob.data(), blob.size(), hipMemcpyHostToDevice, ctx->stream));
	// ---- 1. the items (item_count waits: blob is read by then)
	uint64_t n_items = 0;
	if((rc = item_count(ctx, S, d_ol, n_ol, B, n_items)) != PCR_OK) return rc;
	if(n_items >= POOL_MAX_ITEMS){ g_err = who + ": too many (entry, oligo) hits"; return PCR_ERR_CAPACITY; }
	if(n_items == 0){ zero_rows(); return 0; }
	if((rc = item_fill(ctx, S, d_ol, n_ol, B, n_items)) != PCR_OK) return rc;
	const uint32_t ni = (uint32_t)n_items;
	const unsigned grid_i = (ni + POOL_THREADS - 1)/POOL_THREADS;
	if((rc = X.cnt.ensure((size_t)ni + 1)) != PCR_OK) return rc;                // (the entry counts are spent)
	// ---- with a rule: the 3' end per item (the probes' too: every item has one, the join reads the primers')
	const ItemEnd *d_item_end = nullptr;
	if(ruled && (rc = end3_items(ctx, S, ni, d_ol, d_norm, R.window, use_taq, d_item_end)) != PCR_OK) return rc;
	// ---- 2. job offsets, the jobs; 3. Tm per item
	if((rc = melt_items(who, ctx, S, d_ol, d_olx, ni, args->salt, B)) != PCR_OK) return rc;
	const ItemTm *d_item_tm = (const ItemTm *)X.item_tm.p;
	// ---- 4. the kept products: count (and the rows of the pairs without a probe), scan, compact
	unsigned long long *d_bits = nullptr;
	if(detected){
		if((rc = ctx->pph_bits.ensure(row_words)) != PCR_OK) return rc;
		HIP_TRY(hipMemsetAsync(ctx->pph_bits.p, 0, row_words*sizeof(uint64_t), ctx->stream));
		d_bits = (unsigned long long *)ctx->pph_bits.p;
	}
	const JoinIn J{S.db.p, S.db_cap, S.touched.p, S.d_seg_hi, X.items.p, ni, X.eoff.p, d_ol, n_ol, S.planes.p, S.d_blk_off.p, S.d_len.p,
		S.d_has_eos.p, amp_min, amp_max};
	hipLaunchKernelGGL(k_probe_products<false>, dim3(grid_i), dim3(POOL_THREADS), 0, ctx->stream, J, n_prim, d_item_tm, tm_floor, d_item_end, R, d_intended, d_tab, n_tab,
		d_bits, words, X.cnt.p, (const uint64_t *)nullptr, (uint4 *)nullptr);
	HIP_TRY(hipGetLastError());
	uint64_t n_prod64 = 0;
	if((rc = scan_total(ctx, X.cnt.p, X.ioff, X.tmp, ni, n_prod64)) != PCR_OK) return rc;
	if(n_prod64 >= POOL_MAX_ITEMS){ g_err = who + ": too many products"; return PCR_ERR_CAPACITY; }
	const uint32_t np = (uint32_t)n_prod64;
	uint64_t total = 0;
	unsigned grid_p = 0;
	if(np){
		if((rc = ctx->pph_prod.ensure(np)) != PCR_OK) return rc;
		hipLaunchKernelGGL(k_probe_products<true>, dim3(grid_i), dim3(POOL_THREADS), 0, ctx->stream, J, n_prim, d_item_tm, tm_floor, d_item_end, R, d_intended, d_tab, n_tab,
			(unsigned long long *)nullptr, words, (uint32_t *)nullptr, (const uint64_t *)X.ioff.p, ctx->pph_prod.p);
		HIP_TRY(hipGetLastError());
		// ---- 5. the hits: a wave per product; count (and the rows of the pairs with a probe), scan
		if((rc = ctx->pph_hcnt.ensure((size_t)np + 1)) != PCR_OK) return rc;
		grid_p = std::min<unsigned>((np + PPH_WAVES - 1)/PPH_WAVES, ctx->n_cu*8);
		hipLaunchKernelGGL(k_probe_hits<false>, dim3(grid_p), dim3(64*PPH_WAVES), 0, ctx->stream, S.db.p, S.db_cap, S.d_seg_hi,
			(const uint2 *)X.items.p, (const uint64_t *)X.eoff.p, d_ol, n_ol, n_prim, (const uint4 *)ctx->pph_prod.p, np, d_item_tm, probe_tm_floor,
			d_intended, d_tab, n_tab, d_bits, words, ctx->pph_hcnt.p, (const uint64_t *)nullptr, (pcr_probe_hit *)nullptr, (uint64_t *)nullptr, (uint32_t *)nullptr);
		HIP_TRY(hipGetLastError());
	}
	uint32_t bad = 0;
	auto flag_and_rows = [&]() -> int {
		HIP_TRY(hipMemcpyAsync(&bad, X.flag.p, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
		if(detected) HIP_TRY(hipMemcpyAsync(detected, ctx->pph_bits.p, row_words*sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
		return PCR_OK;
	};
	if(np){ if((rc = scan_total(ctx, ctx->pph_hcnt.p, ctx->pph_hoff, X.tmp, np, total, flag_and_rows)) != PCR_OK) return rc; }
	else{
		if((rc = flag_and_rows()) != PCR_OK) return rc;
		HIP_TRY(hipStreamSynchronize(ctx->stream));
	}
	if(bad & 1u){ g_err = who + ": internal trace-back error"; return PCR_ERR_RANGE; }
	// a pool pair that repeats an earlier assay has that pair's row (the device filled the first copy only)
	for(uint32_t i = 0;i < n_pool && detected;++i)
		if(first_row[i] != i) memcpy(detected + (size_t)i*words, detected + (size_t)first_row[i]*words, words*sizeof(uint64_t));
	if(total >= POOL_MAX_ITEMS){ g_err = who + ": too many hits"; return PCR_ERR_CAPACITY; }
	if(total == 0 || total > cap) return (int64_t)total;                         // count only: out is left as it is
	// ---- 5'. emit at the scanned offsets; 6. the key order
	const uint32_t nr = (uint32_t)total;
	if((rc = ctx->pph_rec.ensure(2*(size_t)nr)) != PCR_OK) return rc;
	if((rc = ctx->pph_keys.ensure(2*(size_t)nr)) != PCR_OK) return rc;
	if((rc = ctx->pph_ord.ensure(2*(size_t)nr)) != PCR_OK) return rc;
	pcr_probe_hit *r0 = ctx->pph_rec.p, *r1 = r0 + nr;
	uint64_t *k0 = ctx->pph_keys.p, *k1 = k0 + nr;
	uint32_t *o0 = ctx->pph_ord.p, *o1 = o0 + nr;
	hipLaunchKernelGGL(k_probe_hits<true>, dim3(grid_p), dim3(64*PPH_WAVES), 0, ctx->stream, S.db.p, S.db_cap, S.d_seg_hi,
		(const uint2 *)X.items.p, (const uint64_t *)X.eoff.p, d_ol, n_ol, n_prim, (const uint4 *)ctx->pph_prod.p, np, d_item_tm, probe_tm_floor,
		d_intended, d_tab, n_tab, (unsigned long long *)nullptr, words, (uint32_t *)nullptr, (const uint64_t *)ctx->pph_hoff.p, r0, k0, o0);
	HIP_TRY(hipGetLastError());
	const unsigned seq_bits = pool_bits(S.n), oligo_bits = pool_bits(n_prim), probe_bits = pool_bits(n_ol - n_prim);
	size_t t0 = 0, t1 = 0, t2 = 0;
	HIP_TRY(rocprim::radix_sort_pairs(nullptr, t0, k0, k1, o0, o1, nr, 0, 33 + probe_bits, ctx->stream));
	HIP_TRY(rocprim::radix_sort_pairs(nullptr, t1, k0, k1, o1, o0, nr, 0, 64, ctx->stream));
	HIP_TRY(rocprim::radix_sort_pairs(nullptr, t2, k0, k1, o0, o1, nr, 0, 2*oligo_bits + seq_bits, ctx->stream));
	if((rc = X.tmp.ensure(std::max(t0, std::max(t1, t2)) + 16)) != PCR_OK) return rc;
	const unsigned grid_r = (nr + 255)/256;
	HIP_TRY(rocprim::radix_sort_pairs(X.tmp.p, t0, k0, k1, o0, o1, nr, 0, 33 + probe_bits, ctx->stream));
	hipLaunchKernelGGL(k_probe_key, dim3(grid_r), dim3(256), 0, ctx->stream, (const pcr_probe_hit *)r0, (const uint32_t *)o1, nr, 1, seq_bits, oligo_bits, k0);
	HIP_TRY(hipGetLastError());
	HIP_TRY(rocprim::radix_sort_pairs(X.tmp.p, t1, k0, k1, o1, o0, nr, 0, 64, ctx->stream));                        // (stable)
	hipLaunchKernelGGL(k_probe_key, dim3(grid_r), dim3(256), 0, ctx->stream, (const pcr_probe_hit *)r0, (const uint32_t *)o0, nr, 2, seq_bits, oligo_bits, k0);
	HIP_TRY(hipGetLastError());
	HIP_TRY(rocprim::radix_sort_pairs(X.tmp.p, t2, k0, k1, o0, o1, nr, 0, 2*oligo_bits + seq_bits, ctx->stream));   // (stable)
	hipLaunchKernelGGL(k_probe_gather, dim3(grid_r), dim3(256), 0, ctx->stream, (const pcr_probe_hit *)r0, (const uint32_t *)o1, nr, r1);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipMemcpyAsync(out, r1, (size_t)nr*sizeof(pcr_probe_hit), hipMemcpyDeviceToHost, ctx->stream));
	HIP_TRY(hipStreamSynchronize(ctx->stream));
	return (int64_t)total;
}

} // namespace

extern "C" {

int64_t pcr_pool_probe_hits(pcr_ctx *ctx, pcr_set which, const pcr_pair *pool, const pcr_word128 *probes, uint32_t n_pool,
	float threshold, int32_t amp_min, int32_t amp_max, const pcr_thermo_args *args, float probe_strand_conc, float template_strand,
	float tm_floor, float probe_tm_floor, uint32_t *oligo_id, uint32_t *probe_id, pcr_probe_hit *out, uint64_t cap,
	uint64_t *detected)
{
	return probe_hits_impl("pcr_pool_probe_hits", ctx, which, pool, probes, n_pool, threshold, amp_min, amp_max, args, probe_strand_conc, template_strand,
		tm_floor, probe_tm_floor, nullptr, oligo_id, probe_id, out, cap, detected);
}

int64_t pcr_pool_probe_hits_end3(pcr_ctx *ctx, pcr_set which, const pcr_pair *pool, const pcr_word128 *probes, uint32_t n_pool,
	float threshold, int32_t amp_min, int32_t amp_max, const pcr_thermo_args *args, float probe_strand_conc, float template_strand,
	float tm_floor, float probe_tm_floor, const pcr_end3_rule *rule, uint32_t *oligo_id, uint32_t *probe_id, pcr_probe_hit *out, uint64_t cap,
	uint64_t *detected)
{
	return probe_hits_impl("pcr_pool_probe_hits_end3", ctx, which, pool, probes, n_pool, threshold, amp_min, amp_max, args, probe_strand_conc,
		template_strand, tm_floor, probe_tm_floor, rule, oligo_id, probe_id, out, cap, detected);
}

} // extern "C"
