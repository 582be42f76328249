// What a primer pool amplifies at every temperature of an annealing gradient, from one melt and one join
// (pcr_pool_anneal_profile; included by pcr_device.hip after pcr_pool.inc and pcr_site_tm.inc, whose stages are its steps 1-3).
//
// The Tm of a site does not depend on the floor pcr_pool_products_tm applies, only the comparison does.  A product with
// v = min(tm_plus, tm_minus) is kept at temps[t] iff !(temps[t] > 0) || v >= temps[t]; temps is strictly ascending, so the kept
// temperatures are a prefix 0 .. u - 1 and u is all a product contributes to the counts.  Per (pool pair, sequence) the highest
// v of the cell's products decides the bit of pcr_pool_products_tm at every floor.
//   1-3. the items, the jobs, k_site_tm, k_item_tm -> item_tm[] (item_count / item_fill, melt_items, on the shared scratch set).
//   4. k_anneal_join: k_products_join's walk (join_walk), no floor.  Per product: u by a binary search in an LDS copy of temps,
//      hist[intended][u] += 1 in LDS (flushed once per block with 64-bit atomic adds), and the cell's melt value raised with an
//      integer atomicMax on the float's bits: v >= +0 (the engine clamps a Tm at 0; v + 0.0f turns a -0 into +0), non-negative
//      floats order like their bit patterns read as int32, and the sentinel -1.0f is a negative int32.  A maximum does not depend
//      on the order of its operands, so the matrices are the same bytes whatever order the threads arrive in.
//      The melt rows are keyed by (plus, minus): row r of `melt` belongs to key_tab[r], the sorted distinct F*n_ol + R and
//      R*n_ol + F of the pool.  melt_fr of pool row i is the row of (F_i, R_i), melt_rf that of (R_i, F_i): pairs that repeat or
//      exchange an earlier one share its rows, F = R has one row for both.  The last row is the spurious vector.
//   5. k_anneal_rows: one workgroup per pool row (and one for the spurious row) streams the row's two melt rows, takes u of
//      max(fr, rf) per sequence into an LDS histogram, and writes the suffix sums: pair_sequences[i][t], cells[t] (atomics),
//      spurious_sequences[t].
//   6. The host turns hist into the points' product counts (products at t = sum of hist[.][u] over u > t).
// The number of launches and copies does not depend on n_temps.  Steps 1-3 work in pcr_ctx::shared, the rest in pcr_ctx::anp_*.
// pcr_pool_anneal_profile_end3 is the same call over the products that pass a 3'-end rule (pcr_products_end3.inc, included before
// this file): k_item_end3 fills an ItemEnd per item before the melt, and the join's functor makes k_end3_join's tests.

namespace {

constexpr uint32_t ANP_BINS = PCR_ANNEAL_MAX_TEMPS + 1;                         // u = 0 .. n_temps
constexpr uint32_t ANP_ROW_THREADS = 256;
// the small results, one u64 array copied back at once: hist[2][ANP_BINS] | cells[MAX_TEMPS] | spurious_sequences[MAX_TEMPS]
constexpr uint32_t ANP_OUT_CELLS = 2*ANP_BINS, ANP_OUT_SPUR = ANP_OUT_CELLS + PCR_ANNEAL_MAX_TEMPS, ANP_OUT_WORDS = ANP_OUT_SPUR + PCR_ANNEAL_MAX_TEMPS;

// The keeping rule, and the number of temperatures of the ascending ts[0 .. n) at which a product with min-Tm v is kept.
__device__ __forceinline__ bool anneal_kept(float v, float t) { return !(t > 0.0f) || v >= t; }
__device__ __forceinline__ uint32_t anneal_prefix(const float *ts, uint32_t n, float v)
{
	uint32_t lo = 0, hi = n;                                                     // kept at every t < lo, at no t >= hi
	while(lo < hi){
		const uint32_t mid = lo + (hi - lo)/2u;
		if(anneal_kept(v, ts[mid])) lo = mid + 1u; else hi = mid;
	}
	return lo;
}

// k_products_join<false> without a floor: one thread per item k, join_walk.  Every product: hist[intended][u], and its cell of
// `melt` (intended: the row of its key) or of the last row (spurious) raised to v.  item_end != NULL: only the products that pass
// the 3'-end rule R (k_end3_join's tests; the rule knows no temperature, so a product that fails it is absent at every one).
__global__ __launch_bounds__(POOL_THREADS) void k_anneal_join(const JoinIn J, const ItemTm *__restrict__ item_tm, const ItemEnd *__restrict__ item_end,
	const End3Rule R, const uint32_t *__restrict__ intended,
	const uint32_t *__restrict__ key_tab, uint32_t n_tab, const float *__restrict__ temps, uint32_t n_temps, int *__restrict__ melt, uint32_t n_seq,
	unsigned long long *__restrict__ out)
{
	__shared__ int2 ss[POOL_MAX_OLIGOS];
	__shared__ float ts[PCR_ANNEAL_MAX_TEMPS];
	__shared__ uint32_t hist[2*ANP_BINS];
	for(uint32_t t = threadIdx.x;t < n_temps;t += blockDim.x) ts[t] = temps[t];
	for(uint32_t b = threadIdx.x;b < 2*ANP_BINS;b += blockDim.x) hist[b] = 0;
	join_geometry(J, ss);
	const uint32_t k = blockIdx.x*blockDim.x + threadIdx.x;
	if(k < J.n_items){                                                           // (no early return: the flush below is the whole block's)
		const uint2 it = J.items[k];
		const uint32_t g = it.x, x = it.y;
		const uint32_t i = J.touched[g/J.cap]*J.cap + g % J.cap;
		const DevEntry ei = J.db[i];
		if(ei.strand == 1){
			const ItemTm tp = item_tm[k];
			ItemEnd ep; ep.clamp3 = ep.end_mismatch = ep.length = ep.pad = 0; ep.id = 0.0f;
			if(item_end) ep = item_end[k];
			const bool plus_ok = !item_end || end3_site_ok(ep, R);
			// (a plus site that fails its own half of the rule keeps no product: it walks nothing)
			if(plus_ok) join_walk<false>(J, ss, g, x, i, ei, 0u, [&](uint64_t t, uint32_t y, uint32_t, int32_t, int32_t, int32_t, int32_t){
				ItemEnd em;
				if(item_end && !end3_product_ok(item_end, R, plus_ok, ep, t, em)) return;
				const ItemTm tm = item_tm[t];
				const float v = ((tp.tm < tm.tm) ? tp.tm : tm.tm) + 0.0f;            // k_products_join's min; + 0.0f: -0 -> +0 (contraction is off)
				const uint32_t u = anneal_prefix(ts, n_temps, v);
				const uint32_t b = x*J.n_ol + y;
				size_t row = n_tab;                                                  // the spurious row
				const bool is_intended = (intended[b >> 5] >> (b & 31)) & 1u;
				if(is_intended){
					uint32_t lo = 0, above = n_tab;                                  // key_tab[lo] <= b < key_tab[above]; an intended b is in the table
					while(above - lo > 1u){
						const uint32_t mid = lo + (above - lo)/2u;
						if(key_tab[mid] <= b) lo = mid; else above = mid;
					}
					row = lo;
				}
				atomicAdd(&hist[(is_intended ? ANP_BINS : 0u) + u], 1u);
				atomicMax(melt + row*n_seq + ei.seq, __float_as_int(v));
			});
		}
	}
	__syncthreads();
	for(uint32_t b = threadIdx.x;b < 2*ANP_BINS;b += blockDim.x){
		const uint32_t c = hist[b];
		if(c) atomicAdd(out + b, (unsigned long long)c);
	}
}

// Workgroup i < n_pool: pool row i, whose melt_fr / melt_rf are rows row_map[i].x / .y of melt; workgroup n_pool: the spurious
// row n_tab.  u of max(fr, rf) per sequence with a product -> LDS histogram -> suffix sums over u.
__global__ __launch_bounds__(ANP_ROW_THREADS) void k_anneal_rows(const int *__restrict__ melt, uint32_t n_seq, const uint2 *__restrict__ row_map,
	uint32_t n_pool, uint32_t n_tab, const float *__restrict__ temps, uint32_t n_temps, uint32_t *__restrict__ pair_seq,
	unsigned long long *__restrict__ out)
{
	__shared__ float ts[PCR_ANNEAL_MAX_TEMPS];
	__shared__ uint32_t hist[ANP_BINS];
	for(uint32_t t = threadIdx.x;t < n_temps;t += blockDim.x) ts[t] = temps[t];
	for(uint32_t b = threadIdx.x;b < ANP_BINS;b += blockDim.x) hist[b] = 0;
	__syncthreads();
	const uint32_t i = blockIdx.x;
	const bool spurious = i >= n_pool;
	const uint2 rows = spurious ? make_uint2(n_tab, n_tab) : row_map[i];
	const int *fr = melt + (size_t)rows.x*n_seq, *rf = melt + (size_t)rows.y*n_seq;
	for(uint32_t s = threadIdx.x;s < n_seq;s += blockDim.x){
		const int a = fr[s], b = rf[s];
		const int m = (a > b) ? a : b;                                           // the order of the floats: see the head of this file
		if(m < 0) continue;                                                      // -1.0f: no product in the cell
		atomicAdd(&hist[anneal_prefix(ts, n_temps, __int_as_float(m))], 1u);
	}
	__syncthreads();
	for(uint32_t t = threadIdx.x;t < n_temps;t += blockDim.x){
		uint32_t c = 0;
		for(uint32_t u = t + 1;u <= n_temps;++u) c += hist[u];                   // kept at t: u > t
		if(spurious) out[ANP_OUT_SPUR + t] = c;
		else{
			pair_seq[(size_t)i*n_temps + t] = c;
			if(c) atomicAdd(out + ANP_OUT_CELLS + t, (unsigned long long)c);
		}
	}
}

// pcr_pool_anneal_profile (rule = NULL) and pcr_pool_anneal_profile_end3; who: the entry point's name, for the refusals
int64_t anneal_profile_impl(const std::string &who, pcr_ctx *ctx, pcr_set which, const pcr_pair *pool, uint32_t n_pool, float threshold,
	int32_t amp_min, int32_t amp_max, const pcr_thermo_args *args, float template_strand, const pcr_end3_rule *rule,
	const float *temps, uint32_t n_temps, uint32_t *oligo_id, pcr_anneal_point *points, uint32_t *pair_sequences,
	float *melt_fr, float *melt_rf, float *melt_spurious)
{
	static_assert(sizeof(pcr_anneal_point) == 40, "record layout");
	static_assert(sizeof(PoolOligo) == 32 && sizeof(SiteOligoX) == 8, "table layout");
	// ---- the arguments, before the handle (pcr_pool_products_tm's checks in its order, the oligo table, then the temperatures)
	if(!set_ok(which)){ g_err = who + ": unknown sequence set"; return PCR_ERR_ARG; }
	if(which != PCR_SET_TARGET && which != PCR_SET_BACKGROUND){ g_err = who + ": PCR_SET_MULTIPLEX is not supported (PCR_SET_TARGET or PCR_SET_BACKGROUND)"; return PCR_ERR_ARG; }
	if(!args || !temps || !points || (n_pool && (!pool || !oligo_id))){ g_err = who + ": bad argument"; return PCR_ERR_ARG; }
	if(n_pool > PCR_POOL_MAX_PAIRS){ g_err = who + ": pool larger than PCR_POOL_MAX_PAIRS"; return PCR_ERR_ARG; }
	if(!(template_strand >= 0.0f) || !(args->primer_strand >= 0.0f)){ g_err = who + ": negative strand concentration (NucCruc::strand, nuc_cruc.h:818-826)"; return PCR_ERR_ARG; }
	if(!(args->salt >= 1.0e-6f && args->salt <= 1.0f)){ g_err = who + ": salt outside [1e-6, 1] (NucCruc::salt, nuc_cruc.h:780-788)"; return PCR_ERR_ARG; }
	std::vector<PoolOligo> ol;
	std::vector<SiteOligoX> olx;
	if(site_oligo_table(who, "an oligo", "primer_strand", pool, n_pool, threshold, args, template_strand, oligo_id, ol, olx) != PCR_OK) return PCR_ERR_ARG;
	if(n_temps == 0 || n_temps > PCR_ANNEAL_MAX_TEMPS){ g_err = who + ": n_temps is 0 or larger than PCR_ANNEAL_MAX_TEMPS"; return PCR_ERR_ARG; }
	for(uint32_t t = 0;t < n_temps;++t){
		if(!std::isfinite(temps[t])){ g_err = who + ": a temperature is not finite"; return PCR_ERR_ARG; }
		if(t && !(temps[t] > temps[t - 1])){ g_err = who + ": temps is not strictly ascending"; return PCR_ERR_ARG; }
	}
	End3Rule R;
	int use_taq;
	if(end3_rule_of(who, rule, R, use_taq) != PCR_OK) return PCR_ERR_ARG;
	const bool ruled = end3_ruled(R);                                            // else: no ItemEnd is computed, the join is the base call's
	if(!ctx){ g_err = who + ": null handle"; return PCR_ERR_ARG; }
	{ const int drc = drain(ctx); if(drc != PCR_OK) return drc; }
	HIP_TRY(hipSetDevice(ctx->device));
	SeqSet &S = ctx->sets[which];
	if(!S.have_db){ g_err = who + ": no word DB (call pcr_select_words or pcr_select_sites first)"; return PCR_ERR_STATE; }
	const size_t n_seq = S.n;
	// whatever the count, everything asked for is written in full: no product anywhere
	auto write_empty = [&](){
		for(uint32_t t = 0;t < n_temps;++t){ pcr_anneal_point p; memset(&p, 0, sizeof p); p.temperature = temps[t]; points[t] = p; }
		if(pair_sequences) memset(pair_sequences, 0, (size_t)n_pool*n_temps*sizeof(uint32_t));
		if(melt_fr) std::fill(melt_fr, melt_fr + (size_t)n_pool*n_seq, PCR_ANNEAL_NO_PRODUCT);
		if(melt_rf) std::fill(melt_rf, melt_rf + (size_t)n_pool*n_seq, PCR_ANNEAL_NO_PRODUCT);
		if(melt_spurious) std::fill(melt_spurious, melt_spurious + n_seq, PCR_ANNEAL_NO_PRODUCT);
	};
	if(n_pool == 0){ write_empty(); return 0; }
	{ const int erc = ensure_touched(ctx, S); if(erc != PCR_OK) return erc; }
	if(S.n_entries == 0 || S.n_touched == 0){ write_empty(); return 0; }
	const uint32_t n_ol = (uint32_t)ol.size();
	// the intended bitmap; the sorted distinct (plus, minus) keys of the pool, one melt row each; each pool row's two rows
	std::vector<uint32_t> intended(((size_t)n_ol*n_ol + 31)/32, 0);
	std::vector<uint32_t> key_tab;
	key_tab.reserve(2*(size_t)n_pool);
	for(uint32_t i = 0;i < n_pool;++i){
		const uint32_t f = oligo_id[2*i], r = oligo_id[2*i + 1];
		for(uint32_t b : {f*n_ol + r, r*n_ol + f}){ intended[b >> 5] |= 1u << (b & 31); key_tab.push_back(b); }
	}
	std::sort(key_tab.begin(), key_tab.end());
	key_tab.erase(std::unique(key_tab.begin(), key_tab.end()), key_tab.end());
	const uint32_t n_tab = (uint32_t)key_tab.size();
	std::vector<uint2> row_map(n_pool);
	for(uint32_t i = 0;i < n_pool;++i){
		const uint32_t f = oligo_id[2*i], r = oligo_id[2*i + 1];
		row_map[i].x = (uint32_t)(std::lower_bound(key_tab.begin(), key_tab.end(), f*n_ol + r) - key_tab.begin());
		row_map[i].y = (uint32_t)(std::lower_bound(key_tab.begin(), key_tab.end(), r*n_ol + f) - key_tab.begin());
	}
	int rc;
	// the melt rows (+ the spurious row) must fit beside what the device already holds: refuse before hipMalloc would fail
	const size_t melt_elems = ((size_t)n_tab + 1)*n_seq;
	if(melt_elems > ctx->anp_melt.cap){
		size_t free_b = 0, total_b = 0;
		HIP_TRY(hipMemGetInfo(&free_b, &total_b));
		const size_t have = free_b + ctx->anp_melt.cap*sizeof(float);             // (ensure gives the old buffer back first)
		const size_t headroom = size_t(256) << 20;
		if(have < headroom || melt_elems*sizeof(float) > have - headroom){
			g_err = who + ": the melt rows of the pool's distinct (F, R) would not fit in device memory"; return PCR_ERR_CAPACITY;
		}
	}
	if((rc = ctx->anp_melt.ensure(melt_elems)) != PCR_OK) return rc;
	const size_t ol_bytes = ol.size()*sizeof(PoolOligo), olx_bytes = olx.size()*sizeof(SiteOligoX), map_bytes = row_map.size()*sizeof(uint2),
		tab_bytes = key_tab.size()*sizeof(uint32_t), int_bytes = intended.size()*sizeof(uint32_t), temp_bytes = (size_t)n_temps*sizeof(float);
	const std::vector<float> norm = ruled ? end3_norms(ol) : std::vector<float>();   // (k_item_end3's; only a rule reads it)
	const size_t norm_bytes = norm.size()*sizeof(float);
	std::vector<uint8_t> blob(ol_bytes + olx_bytes + map_bytes + tab_bytes + int_bytes + temp_bytes + norm_bytes);   // 32-, 8-, 8-, 4-, 4-, 4- and 4-byte records, in that order: each is aligned
	memcpy(blob.data(), ol.data(), ol_bytes);
	memcpy(blob.data() + ol_bytes, olx.data(), olx_bytes);
	memcpy(blob.data() + ol_bytes + olx_bytes, row_map.data(), map_bytes);
	memcpy(blob.data() + ol_bytes + olx_bytes + map_bytes, key_tab.data(), tab_bytes);
	memcpy(blob.data() + ol_bytes + olx_bytes + map_bytes + tab_bytes, intended.data(), int_bytes);
	memcpy(blob.data() + ol_bytes + olx_bytes + map_bytes + tab_bytes + int_bytes, temps, temp_bytes);
	if(norm_bytes) memcpy(blob.data() + ol_bytes + olx_bytes + map_bytes + tab_bytes + int_bytes + temp_bytes, norm.data(), norm_bytes);
	ItemScratch &X = ctx->shared;
	const ItemBufs B = X.bufs();
	if((rc = X.in.ensure(blob.size())) != PCR_OK) return rc;
	const PoolOligo *d_ol = (const PoolOligo *)X.in.p;
	const SiteOligoX *d_olx = (const SiteOligoX *)(X.in.p + ol_bytes);
	const uint2 *d_map = (const uint2 *)(X.in.p + ol_bytes + olx_bytes);
	const uint32_t *d_tab = (const uint32_t *)(X.in.p + ol_bytes + olx_bytes + map_bytes);
	const uint32_t *d_intended = (const uint32_t *)(X.in.p + ol_bytes + olx_bytes + map_bytes + tab_bytes);
	const float *d_temps = (const float *)(X.in.p + ol_bytes + olx_bytes + map_bytes + tab_bytes + int_bytes);
	const float *d_norm = (const float *)(X.in.p + ol_bytes + olx_bytes + map_bytes + tab_bytes + int_bytes + temp_bytes);
	HIP_TRY(hipMemcpyAsync(X.in.p, blob.data(), blob.size(), hipMemcpyHostToDevice, ctx->stream));
	// ---- 1. the items (item_count waits: blob is read by then)
	uint64_t n_items = 0;
	if((rc = item_count(ctx, S, d_ol, n_ol, B, n_items)) != PCR_OK) return rc;
	if(n_items >= POOL_MAX_ITEMS){ g_err = who + ": too many (entry, oligo) hits"; return PCR_ERR_CAPACITY; }
	if(n_items == 0){ write_empty(); return 0; }
	if((rc = item_fill(ctx, S, d_ol, n_ol, B, n_items)) != PCR_OK) return rc;
	const uint32_t ni = (uint32_t)n_items;
	const unsigned grid_i = (ni + POOL_THREADS - 1)/POOL_THREADS;
	if((rc = X.cnt.ensure((size_t)ni + 1)) != PCR_OK) return rc;                // (the entry counts are spent)
	// ---- with a rule: the 3' end per item (pcr_pool_products_end3's step 2)
	const ItemEnd *d_item_end = nullptr;
	if(ruled && (rc = end3_items(ctx, S, ni, d_ol, d_norm, R.window, use_taq, d_item_end)) != PCR_OK) return rc;
	// ---- 2. job offsets, the jobs; 3. Tm per item
	if((rc = melt_items(who, ctx, S, d_ol, d_olx, ni, args->salt, B)) != PCR_OK) return rc;
	// ---- 4. the join: histograms and melt rows
	if((rc = ctx->anp_out.ensure(ANP_OUT_WORDS)) != PCR_OK) return rc;
	if((rc = ctx->anp_pairseq.ensure((size_t)n_pool*n_temps)) != PCR_OK) return rc;
	HIP_TRY(hipMemsetAsync(ctx->anp_out.p, 0, ANP_OUT_WORDS*sizeof(uint64_t), ctx->stream));
	HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)ctx->anp_melt.p, (int)0xBF800000u, melt_elems, ctx->stream));   // -1.0f
	const JoinIn J{S.db.p, S.db_cap, S.touched.p, S.d_seg_hi, X.items.p, ni, X.eoff.p, d_ol, n_ol, S.planes.p, S.d_blk_off.p, S.d_len.p,
		S.d_has_eos.p, amp_min, amp_max};
	hipLaunchKernelGGL(k_anneal_join, dim3(grid_i), dim3(POOL_THREADS), 0, ctx->stream, J, (const ItemTm *)X.item_tm.p, d_item_end, R, d_intended, d_tab, n_tab,
		d_temps, n_temps, (int *)ctx->anp_melt.p, (uint32_t)n_seq, (unsigned long long *)ctx->anp_out.p);
	HIP_TRY(hipGetLastError());
	// ---- 5. the rows' histograms
	hipLaunchKernelGGL(k_anneal_rows, dim3(n_pool + 1), dim3(ANP_ROW_THREADS), 0, ctx->stream, (const int *)ctx->anp_melt.p, (uint32_t)n_seq,
		d_map, n_pool, n_tab, d_temps, n_temps, ctx->anp_pairseq.p, (unsigned long long *)ctx->anp_out.p);
	HIP_TRY(hipGetLastError());
	uint64_t small[ANP_OUT_WORDS];
	uint32_t bad = 0;
	const bool want_rows = melt_fr || melt_rf;
	std::vector<float> host_melt;                                               // the keyed rows (+ the spurious row), when a matrix is asked for
	HIP_TRY(hipMemcpyAsync(small, ctx->anp_out.p, sizeof small, hipMemcpyDeviceToHost, ctx->stream));
	HIP_TRY(hipMemcpyAsync(&bad, X.flag.p, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
	if(pair_sequences) HIP_TRY(hipMemcpyAsync(pair_sequences, ctx->anp_pairseq.p, (size_t)n_pool*n_temps*sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
	if(want_rows){
		host_melt.resize(melt_elems);
		HIP_TRY(hipMemcpyAsync(host_melt.data(), ctx->anp_melt.p, melt_elems*sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
	}
	else if(melt_spurious) HIP_TRY(hipMemcpyAsync(melt_spurious, ctx->anp_melt.p + (size_t)n_tab*n_seq, n_seq*sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
	HIP_TRY(hipStreamSynchronize(ctx->stream));
	if(bad & 1u){ g_err = who + ": internal trace-back error"; return PCR_ERR_RANGE; }
	uint64_t total = 0;
	for(uint32_t b = 0;b < 2*ANP_BINS;++b) total += small[b];
	if(total >= POOL_MAX_ITEMS){ g_err = who + ": too many products"; return PCR_ERR_CAPACITY; }
	// ---- 6. the points: a product with u kept temperatures counts at every t < u
	uint64_t kept[2] = {0, 0};
	for(uint32_t t = n_temps;t-- > 0;){
		for(int c = 0;c < 2;++c) kept[c] += small[c*ANP_BINS + t + 1];
		pcr_anneal_point p;
		p.temperature = temps[t]; p.reserved = 0;
		p.products_spurious = kept[0]; p.products_intended = kept[1];
		p.cells = small[ANP_OUT_CELLS + t]; p.spurious_sequences = small[ANP_OUT_SPUR + t];
		points[t] = p;
	}
	if(want_rows){
		for(uint32_t i = 0;i < n_pool;++i){
			if(melt_fr) memcpy(melt_fr + (size_t)i*n_seq, host_melt.data() + (size_t)row_map[i].x*n_seq, n_seq*sizeof(float));
			if(melt_rf) memcpy(melt_rf + (size_t)i*n_seq, host_melt.data() + (size_t)row_map[i].y*n_seq, n_seq*sizeof(float));
		}
		if(melt_spurious) memcpy(melt_spurious, host_melt.data() + (size_t)n_tab*n_seq, n_seq*sizeof(float));
	}
	return (int64_t)total;
}

} // namespace

extern "C" {

int64_t pcr_pool_anneal_profile(pcr_ctx *ctx, pcr_set which, const pcr_pair *pool, uint32_t n_pool, float threshold,
	int32_t amp_min, int32_t amp_max, const pcr_thermo_args *args, float template_strand,
	const float *temps, uint32_t n_temps, uint32_t *oligo_id, pcr_anneal_point *points, uint32_t *pair_sequences,
	float *melt_fr, float *melt_rf, float *melt_spurious)
{
	return anneal_profile_impl("pcr_pool_anneal_profile", ctx, which, pool, n_pool, threshold, amp_min, amp_max, args, template_strand, nullptr,
		temps, n_temps, oligo_id, points, pair_sequences, melt_fr, melt_rf, melt_spurious);
}

int64_t pcr_pool_anneal_profile_end3(pcr_ctx *ctx, pcr_set which, const pcr_pair *pool, uint32_t n_pool, float threshold,
	int32_t amp_min, int32_t amp_max, const pcr_thermo_args *args, float template_strand, const pcr_end3_rule *rule,
	const float *temps, uint32_t n_temps, uint32_t *oligo_id, pcr_anneal_point *points, uint32_t *pair_sequences,
	float *melt_fr, float *melt_rf, float *melt_spurious)
{
	return anneal_profile_impl("pcr_pool_anneal_profile_end3", ctx, which, pool, n_pool, threshold, amp_min, amp_max, args, template_strand, rule,
		temps, n_temps, oligo_id, points, pair_sequences, melt_fr, melt_rf, melt_spurious);
}

} // extern "C"
