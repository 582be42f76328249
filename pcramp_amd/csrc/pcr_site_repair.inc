// Degenerate bases that win back a panel's eroded binding sites (pcr_site_repair; included by pcr_device.hip after
// pcr_site_variants.inc, whose checks and pipeline -- sv_check, sv_run -- it calls for the sites, the variants and their order).
//
// After sv_run(args = NULL) the device holds the items in key order with the scan of their head flags, every variant's first
// position and its place in record order.  On top of that:
//   1. k_rp_variants: per record f the variant's footprint (its planes at the oligo's slots) and its sites; k_rp_bounds<false>: where
//      each oligo's records begin (records are sorted by oligo first).
//   2. k_rp_pairs: one (oligo, sequence) key and one record index per position that opens a sequence of its variant -- the
//      distinct (variant, sequence) pairs -- and one stable radix sort by (oligo, sequence).  k_rp_heads + a scan: a pair opens a
//      sequence run where the key changes; k_rp_runs: where each run starts; k_rp_bounds<true>: where each oligo's runs begin.
//      The held bitset has one bit per run, an oligo's bits being consecutive.
//   3. k_rp_step<true>: a workgroup per oligo: W = the oligo, what it holds, the bitset, the record of step 0.
//   4. Per step, all oligos in the same three launches, the host waiting once for the number of oligos still going:
//      k_rp_candidates  a workgroup per oligo walks its records in order and compacts the first max_candidates that W does not
//                       hold, that are single-base and whose union stays within max_degeneracy (ballot + prefix: record order kept);
//      k_rp_weigh       a workgroup per (oligo, candidate): W' = W | footprint; every variant of the oligo against W' (sites and
//                       variants held), then every sequence run not yet held against W' (the gain); wave shuffles, then LDS;
//      k_rp_step<false> a workgroup per oligo: the arg-max by (gain, sites held) descending, (expansions, record) ascending -- a
//                       total order --, the union, what it holds, the bitset, the step's record and the reason to stop.
//   5. The records of all oligos come back in one copy; with thermodynamics their words go through pcr_thermo in one batch.
// Whether W' holds a variant is four ANDs, three ORs and a popcount on a 16-byte footprint, so k_rp_weigh computes it where it
// needs it (the footprints of an oligo stay in L2) instead of keeping a bitmap per workgroup: no size of an oligo's variant
// list is special.  Integer atomics only (the bitset's 64-bit words, which two oligos can share, and the count of oligos still going); no hash.
// All scratch is pcr_ctx::rp_* (and site_tmp for rocprim); nothing is kept in it between calls.

namespace {

constexpr uint32_t RP_SLOTS = PCR_REPAIR_MAX_STEPS + 1;                       // records per oligo at most
constexpr uint32_t RP_SATURATED = 1u << 20;                                   // any degeneracy above every legal max_degeneracy

struct RpState { Planes w; uint32_t seq_held, step, stop, n_cand, any_single, pad[3]; };   // an oligo between the launches
struct RpScore { uint32_t gain, sites, variants, n_exp; };                    // a candidate's union, weighed
struct RpRule { uint32_t max_degeneracy, max_mismatch, clamp3, max_candidates, max_steps; };

__device__ __forceinline__ uint32_t rp_slot_mask(const PoolOligo &o)
{
	const uint32_t upto = (o.stop >= 31) ? 0xFFFFFFFFu : ((1u << (o.stop + 1)) - 1u);
	return upto & ~((1u << o.start) - 1u);
}

// the slots stop-clamp3+1 .. stop; all of them (so that nothing is held) where clamp3 exceeds the oligo's length
__device__ __forceinline__ uint32_t rp_clamp_mask(const PoolOligo &o, uint32_t clamp3, bool &never)
{
	const uint32_t len = (uint32_t)(o.stop - o.start + 1);
	never = clamp3 > len;
	if(clamp3 == 0 || never) return 0u;
	const uint32_t upto = (o.stop >= 31) ? 0xFFFFFFFFu : ((1u << (o.stop + 1)) - 1u);
	const uint32_t lo = (uint32_t)o.stop + 1u - clamp3;
	return upto & ~((1u << lo) - 1u);
}

__device__ __forceinline__ bool rp_holds(const Planes &w, const uint4 v, uint32_t mask, uint32_t clamp, bool never, uint32_t max_mismatch)
{
	const uint32_t miss = ~((v.x & w.a) | (v.y & w.c) | (v.z & w.g) | (v.w & w.t)) & mask;
	return !never && (uint32_t)__popc(miss) <= max_mismatch && !(miss & clamp);
}

__device__ __forceinline__ bool rp_single(const uint4 v, uint32_t mask)
{
	const uint32_t any = v.x | v.y | v.z | v.w;
	return any == mask && (uint32_t)(__popc(v.x) + __popc(v.y) + __popc(v.z) + __popc(v.w)) == (uint32_t)__popc(mask);
}

// Word::degeneracy(), saturating above every legal bound
__device__ __forceinline__ uint32_t rp_degeneracy(const Planes &w, const PoolOligo &o)
{
	uint32_t d = 1;
	for(int k = o.start;k <= o.stop;++k){
		const uint32_t n = ((w.a >> k) & 1u) + ((w.c >> k) & 1u) + ((w.g >> k) & 1u) + ((w.t >> k) & 1u);
		d = min(d*n, RP_SATURATED);
	}
	return d;
}

__device__ __forceinline__ Planes rp_union(const Planes &w, const uint4 v)
{
	Planes u; u.a = w.a | v.x; u.c = w.c | v.y; u.g = w.g | v.z; u.t = w.t | v.w;
	return u;
}

// record f (record order) <- variant v (key order): the footprint and the sites
__global__ __launch_bounds__(POOL_THREADS) void k_rp_variants(const SvItem *__restrict__ sv, const uint32_t *__restrict__ ord,
	const uint32_t *__restrict__ start, const uint32_t *__restrict__ rank, uint32_t n_var, const PoolOligo *__restrict__ oligos,
	uint4 *__restrict__ foot, uint32_t *__restrict__ sites)
{
	const uint32_t v = blockIdx.x*blockDim.x + threadIdx.x;
	if(v >= n_var) return;
	const uint32_t s0 = start[v], f = rank[v];
	const SvItem it = sv[ord[s0]];
	const uint32_t m = rp_slot_mask(oligos[it.oligo]);
	foot[f] = make_uint4(it.w.a & m, it.w.c & m, it.w.g & m, it.w.t & m);
	sites[f] = start[v + 1] - s0;
}

// first[o] = the first of n ascending elements whose oligo is at least o (o = 0 .. n_ol): the oligo of a record, or of a pair's
// key; RUNS: that pair's run instead (it opens one), n_runs past the end
template<bool RUNS>
__global__ __launch_bounds__(POOL_THREADS) void k_rp_bounds(const pcr_site_variant *__restrict__ rec, const uint64_t *__restrict__ key, uint32_t seq_bits,
	const uint32_t *__restrict__ run_sum, uint32_t n, uint32_t n_ol, uint32_t *__restrict__ first)
{
	const uint32_t o = blockIdx.x*blockDim.x + threadIdx.x;
	if(o > n_ol) return;
	uint32_t lo = 0, hi = n;                                                    // elements below lo are < o, elements from hi on are >= o
	while(lo < hi){
		const uint32_t mid = lo + (hi - lo)/2u;
		const uint32_t x = RUNS ? (uint32_t)(key[mid] >> seq_bits) : rec[mid].oligo;
		if(x < o) lo = mid + 1u; else hi = mid;
	}
	first[o] = RUNS ? ((lo < n) ? run_sum[lo] - 1u : run_sum[n - 1]) : lo;
}

// position s of the key order opens a sequence of its variant: pair (high half of the scan) - 1
__global__ __launch_bounds__(POOL_THREADS) void k_rp_pairs(const SvItem *__restrict__ sv, const uint32_t *__restrict__ ord, const uint64_t *__restrict__ sum,
	const uint32_t *__restrict__ rank, uint32_t n_items, uint32_t seq_bits, uint64_t *__restrict__ key, uint32_t *__restrict__ val)
{
	const uint32_t s = blockIdx.x*blockDim.x + threadIdx.x;
	if(s >= n_items) return;
	const uint64_t x = sum[s];
	if(s > 0 && (uint32_t)(sum[s - 1] >> 32) == (uint32_t)(x >> 32)) return;
	const SvItem it = sv[ord[s]];
	const uint32_t p = (uint32_t)(x >> 32) - 1u;
	key[p] = ((uint64_t)it.oligo << seq_bits) | it.seq;
	val[p] = rank[(uint32_t)x - 1u];
}

__global__ __launch_bounds__(POOL_THREADS) void k_rp_heads(const uint64_t *__restrict__ key, uint32_t n, uint32_t *__restrict__ flag)
{
	const uint32_t p = blockIdx.x*blockDim.x + threadIdx.x;
	if(p < n) flag[p] = (p == 0 || key[p] != key[p - 1]) ? 1u : 0u;
}

// run_sum: the inclusive scan of the heads.  Run r = run_sum - 1 starts where it steps; run_start[n_runs] = n.
__global__ __launch_bounds__(POOL_THREADS) void k_rp_runs(const uint32_t *__restrict__ run_sum, uint32_t n, uint32_t *__restrict__ run_start)
{
	const uint32_t p = blockIdx.x*blockDim.x + threadIdx.x;
	if(p >= n) return;
	if(p == 0 || run_sum[p - 1] != run_sum[p]) run_start[run_sum[p] - 1u] = p;
	if(p == n - 1) run_start[run_sum[p]] = n;
}

// the sum of x over the workgroup, for every thread (POOL_THREADS threads; part: POOL_THREADS/64 words of LDS)
__device__ __forceinline__ uint32_t rp_block_sum(uint32_t x, uint32_t *part)
{
	for(int d = 32;d > 0;d >>= 1) x += __shfl_down(x, d, 64);
	__syncthreads();                                                            // part may still be read from the sum before
	if((threadIdx.x & 63u) == 0) part[threadIdx.x >> 6] = x;
	__syncthreads();
	uint32_t s = 0;
	for(int w = 0;w < POOL_THREADS/64;++w) s += part[w];
	return s;
}

// Oligo blockIdx.x: the first max_candidates records, in order, that its W does not hold, that are single-base and whose union
// stays within max_degeneracy; whether any unheld single-base record exists (known whenever the list stays empty).
__global__ __launch_bounds__(POOL_THREADS) void k_rp_candidates(const PoolOligo *__restrict__ oligos, const uint32_t *__restrict__ var_first,
	const uint4 *__restrict__ foot, const RpRule rule, RpState *__restrict__ state, uint32_t *__restrict__ cand)
{
	__shared__ uint32_t wave_n[POOL_THREADS/64];
	__shared__ uint32_t single;
	const uint32_t o = blockIdx.x;
	RpState &st = state[o];
	if(st.stop) return;                                                         // uniform: written by an earlier launch
	const PoolOligo ol = oligos[o];
	const Planes w = st.w;
	bool never;
	const uint32_t mask = rp_slot_mask(ol), clamp = rp_clamp_mask(ol, rule.clamp3, never);
	const uint32_t f0 = var_first[o], f1 = var_first[o + 1];
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	if(threadIdx.x == 0) single = 0;
	uint32_t base = 0;
	for(uint32_t c0 = f0;c0 < f1 && base < rule.max_candidates;c0 += POOL_THREADS){   // uniform
		const uint32_t f = c0 + threadIdx.x;
		bool take = false, open = false;
		if(f < f1){
			const uint4 v = foot[f];
			open = !rp_holds(w, v, mask, clamp, never, rule.max_mismatch) && rp_single(v, mask);
			take = open && rp_degeneracy(rp_union(w, v), ol) <= rule.max_degeneracy;
		}
		const unsigned long long b = __ballot(take);
		__syncthreads();                                                         // wave_n of the chunk before has been read
		if(lane == 0) wave_n[wave] = (uint32_t)__popcll(b);
		if(open) single = 1u;
		__syncthreads();
		uint32_t before = base, total = 0;
		for(uint32_t k = 0;k < (uint32_t)(POOL_THREADS/64);++k){ if(k < wave) before += wave_n[k]; total += wave_n[k]; }
		const uint32_t at = before + (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
		if(take && at < rule.max_candidates) cand[(size_t)o*rule.max_candidates + at] = f;
		base += total;
	}
	__syncthreads();
	if(threadIdx.x == 0){ st.n_cand = min(base, rule.max_candidates); st.any_single = single; }
}

// Candidate blockIdx.x of oligo blockIdx.y: what W | footprint holds.
__global__ __launch_bounds__(POOL_THREADS) void k_rp_weigh(const PoolOligo *__restrict__ oligos, const uint32_t *__restrict__ var_first,
	const uint4 *__restrict__ foot, const uint32_t *__restrict__ sites, const uint32_t *__restrict__ run_first, const uint32_t *__restrict__ run_start,
	const uint32_t *__restrict__ pair_var, const uint64_t *__restrict__ held, const RpRule rule, const RpState *__restrict__ state,
	const uint32_t *__restrict__ cand, RpScore *__restrict__ score)
{
	__shared__ uint32_t part[POOL_THREADS/64];
	const uint32_t o = blockIdx.y, c = blockIdx.x;
	const RpState &st = state[o];
	if(st.stop || c >= st.n_cand) return;                                       // uniform
	const PoolOligo ol = oligos[o];
	bool never;
	const uint32_t mask = rp_slot_mask(ol), clamp = rp_clamp_mask(ol, rule.clamp3, never);
	const Planes w = rp_union(st.w, foot[cand[(size_t)o*rule.max_candidates + c]]);
	uint32_t n_sites = 0, n_var = 0, gain = 0;
	for(uint32_t f = var_first[o] + threadIdx.x;f < var_first[o + 1];f += POOL_THREADS){
		if(rp_holds(w, foot[f], mask, clamp, never, rule.max_mismatch)){ n_sites += sites[f]; ++n_var; }
	}
	for(uint32_t r = run_first[o] + threadIdx.x;r < run_first[o + 1];r += POOL_THREADS){
		if((held[r >> 6] >> (r & 63u)) & 1ull) continue;
		bool got = false;
		for(uint32_t p = run_start[r];p < run_start[r + 1] && !got;++p) got = rp_holds(w, foot[pair_var[p]], mask, clamp, never, rule.max_mismatch);
		gain += got ? 1u : 0u;
	}
	n_sites = rp_block_sum(n_sites, part);
	n_var = rp_block_sum(n_var, part);
	gain = rp_block_sum(gain, part);
	if(threadIdx.x == 0){
		RpScore s; s.gain = gain; s.sites = n_sites; s.variants = n_var; s.n_exp = rp_degeneracy(w, ol);
		score[(size_t)o*rule.max_candidates + c] = s;
	}
}

// x before y in the step's total order: gain, then sites held descending; expansions, then record ascending
__device__ __forceinline__ bool rp_better(const RpScore &x, uint32_t fx, const RpScore &y, uint32_t fy)
{
	if(x.gain != y.gain) return x.gain > y.gain;
	if(x.sites != y.sites) return x.sites > y.sites;
	if(x.n_exp != y.n_exp) return x.n_exp < y.n_exp;
	return fx < fy;
}

// Oligo blockIdx.x.  FIRST: step 0, W = the oligo.  Otherwise the step: pick, union, or stop with the reason on the last record.
// Then what W holds, the bitset, the record, and whether the oligo goes on (counted in *going).
template<bool FIRST>
__global__ __launch_bounds__(POOL_THREADS) void k_rp_step(const PoolOligo *__restrict__ oligos, const uint32_t *__restrict__ var_first,
	const uint4 *__restrict__ foot, const uint32_t *__restrict__ sites, const uint32_t *__restrict__ run_first, const uint32_t *__restrict__ run_start,
	const uint32_t *__restrict__ pair_var, uint64_t *__restrict__ held, const RpRule rule, RpState *__restrict__ state,
	const uint32_t *__restrict__ cand, const RpScore *__restrict__ score, pcr_repair_step *__restrict__ rec, uint32_t *__restrict__ going)
{
	__shared__ uint32_t part[POOL_THREADS/64];
	__shared__ uint32_t best_c[POOL_THREADS];
	const uint32_t o = blockIdx.x;
	RpState &st = state[o];
	const PoolOligo ol = oligos[o];
	Planes w = ol.m;
	uint32_t step = 0, variant = PCR_REPAIR_NO_VARIANT, added = 0, n_cand = 0, gain = 0;
	if(!FIRST){
		if(st.stop) return;                                                      // uniform
		n_cand = st.n_cand; step = st.step; w = st.w;
		// the arg-max: every thread over its candidates, then a tree over the threads' winners
		uint32_t mine = 0xFFFFFFFFu;
		for(uint32_t c = threadIdx.x;c < n_cand;c += POOL_THREADS){
			if(mine == 0xFFFFFFFFu || rp_better(score[(size_t)o*rule.max_candidates + c], cand[(size_t)o*rule.max_candidates + c],
				score[(size_t)o*rule.max_candidates + mine], cand[(size_t)o*rule.max_candidates + mine])) mine = c;
		}
		best_c[threadIdx.x] = mine;
		__syncthreads();
		for(uint32_t d = POOL_THREADS/2;d > 0;d >>= 1){
			if(threadIdx.x < d){
				const uint32_t x = best_c[threadIdx.x], y = best_c[threadIdx.x + d];
				if(y != 0xFFFFFFFFu && (x == 0xFFFFFFFFu || rp_better(score[(size_t)o*rule.max_candidates + y], cand[(size_t)o*rule.max_candidates + y],
					score[(size_t)o*rule.max_candidates + x], cand[(size_t)o*rule.max_candidates + x]))) best_c[threadIdx.x] = y;
			}
			__syncthreads();
		}
		const uint32_t best = best_c[0];
		const uint32_t best_gain = (best == 0xFFFFFFFFu) ? 0u : score[(size_t)o*rule.max_candidates + best].gain;
		if(best_gain == 0){                                                      // uniform: nothing to take, the record before was the last
			if(threadIdx.x == 0){
				st.stop = (n_cand == 0 && st.any_single) ? PCR_REPAIR_DEGENERACY : PCR_REPAIR_NO_GAIN;
				rec[(size_t)o*RP_SLOTS + step].flags = st.stop;
			}
			return;
		}
		variant = cand[(size_t)o*rule.max_candidates + best];
		const Planes u = rp_union(w, foot[variant]);
		added = ((u.a ^ w.a) | (u.c ^ w.c) | (u.g ^ w.g) | (u.t ^ w.t)) >> ol.start;
		w = u; gain = best_gain; ++step;
	}
	bool never;
	const uint32_t mask = rp_slot_mask(ol), clamp = rp_clamp_mask(ol, rule.clamp3, never);
	uint32_t n_sites = 0, n_var = 0, n_seq = 0;
	for(uint32_t f = var_first[o] + threadIdx.x;f < var_first[o + 1];f += POOL_THREADS){
		if(rp_holds(w, foot[f], mask, clamp, never, rule.max_mismatch)){ n_sites += sites[f]; ++n_var; }
	}
	const uint32_t r0 = run_first[o], r1 = run_first[o + 1];
	for(uint32_t r = r0 + threadIdx.x;r < r1;r += POOL_THREADS){
		bool got = false;
		for(uint32_t p = run_start[r];p < run_start[r + 1] && !got;++p) got = rp_holds(w, foot[pair_var[p]], mask, clamp, never, rule.max_mismatch);
		if(got){ ++n_seq; atomicOr((unsigned long long *)&held[r >> 6], 1ull << (r & 63u)); }   // (a word may be shared with the next oligo)
	}
	n_sites = rp_block_sum(n_sites, part);
	n_var = rp_block_sum(n_var, part);
	n_seq = rp_block_sum(n_seq, part);
	if(threadIdx.x != 0) return;
	const uint32_t total = r1 - r0;
	const uint32_t stop = (n_seq == total) ? PCR_REPAIR_COMPLETE : (step == rule.max_steps) ? PCR_REPAIR_STEPS : 0u;
	pcr_repair_step r;
	r.word.w[0] = r.word.w[1] = 0ull;
	for(uint32_t k = 0;k < 32u;++k){                                              // word.cpp:11-16, as k_sv_records
		const uint64_t nib = ((w.a >> k) & 1u) | (((w.c >> k) & 1u) << 1) | (((w.g >> k) & 1u) << 2) | (((w.t >> k) & 1u) << 3);
		r.word.w[k >> 4] |= nib << ((15u - (k & 15u))*4u);
	}
	r.oligo = o; r.step = step; r.variant = variant; r.added_mask = added; r.n_expansions = rp_degeneracy(w, ol);
	r.candidates = n_cand; r.sequences_held = n_seq; r.sites_held = n_sites; r.variants_held = n_var; r.sequences_total = total;
	r.gain = gain; r.flags = stop; r.valid = 0; r.reserved = 0;
	rec[(size_t)o*RP_SLOTS + step] = r;
	st.w = w; st.seq_held = n_seq; st.step = step; st.stop = stop; st.n_cand = 0; st.any_single = 0;
	if(!stop) atomicAdd(going, 1u);
}

// the word of an oligo's planes (word.cpp:11-16)
void rp_word_of(const Planes &m, pcr_word128 &out)
{
	out.w[0] = out.w[1] = 0;
	for(int k = 0;k < 32;++k)
		pcrhost::word_set(out.w, k, ((m.a >> k) & 1u) | (((m.c >> k) & 1u) << 1) | (((m.g >> k) & 1u) << 2) | (((m.t >> k) & 1u) << 3));
}

} // namespace

extern "C" {

int64_t pcr_site_repair(pcr_ctx *ctx, pcr_set which, const pcr_pair *pairs, uint32_t n_pairs, float threshold,
	uint32_t max_degeneracy, uint32_t max_mismatch, uint32_t clamp3, uint32_t max_candidates, uint32_t max_steps,
	const pcr_thermo_args *args, int check_homo_dimer, uint32_t *oligo_id, pcr_repair_step *out, uint64_t cap)
{
	static_assert(sizeof(pcr_repair_step) == 72, "record layout");
	static_assert(sizeof(RpState) == 48 && sizeof(RpScore) == 16, "scratch layout");
	// ---- the arguments, before the handle
	std::vector<PoolOligo> ol;
	std::vector<SiteOligoX> olx;
	int rc = sv_check("pcr_site_repair", which, pairs, n_pairs, threshold, args, 0.0f, oligo_id, cap && !out, ol, olx);
	if(rc != PCR_OK) return rc;
	if(max_degeneracy == 0 || max_degeneracy > PCR_SITE_MAX_EXPANSIONS){ g_err = "pcr_site_repair: max_degeneracy is 0 or above PCR_SITE_MAX_EXPANSIONS"; return PCR_ERR_ARG; }
	if(clamp3 > 32){ g_err = "pcr_site_repair: clamp3 above 32"; return PCR_ERR_ARG; }
	if(max_candidates == 0 || max_candidates > PCR_REPAIR_MAX_CANDIDATES){ g_err = "pcr_site_repair: max_candidates is 0 or above PCR_REPAIR_MAX_CANDIDATES"; return PCR_ERR_ARG; }
	if(max_steps > PCR_REPAIR_MAX_STEPS){ g_err = "pcr_site_repair: max_steps above PCR_REPAIR_MAX_STEPS"; return PCR_ERR_ARG; }
	// ---- the sites and the variants (no thermodynamics: the record order does not depend on it)
	SvRun run;
	const int64_t nv64 = sv_run("pcr_site_repair", ctx, which, n_pairs, nullptr, ol, olx, 0, true, nullptr, run);
	if(nv64 < 0) return nv64;
	if(n_pairs == 0) return 0;
	const uint32_t n_ol = (uint32_t)ol.size();
	std::vector<pcr_repair_step> recs;
	if(!run.done){                                                                // no site at all: every oligo's step 0, nothing to hold
		for(uint32_t o = 0;o < n_ol;++o){
			pcr_repair_step r; memset(&r, 0, sizeof(r));
			rp_word_of(ol[o].m, r.word);
			r.oligo = o; r.variant = PCR_REPAIR_NO_VARIANT; r.n_expansions = olx[o].n_exp; r.flags = PCR_REPAIR_COMPLETE;
			recs.push_back(r);
		}
	}
	else{
		const uint32_t ni = run.ni, nv = run.nv, np = run.n_vseq;                // np: 1 .. ni
		SeqSet &S = ctx->sets[which];
		const unsigned seq_bits = pool_bits(S.n), oligo_bits = pool_bits(n_ol);
		const unsigned grid_i = (ni + POOL_THREADS - 1)/POOL_THREADS, grid_v = (nv + POOL_THREADS - 1)/POOL_THREADS;
		const unsigned grid_p = (np + POOL_THREADS - 1)/POOL_THREADS, grid_o = (n_ol + 1 + POOL_THREADS - 1)/POOL_THREADS;
		const size_t held_words = (size_t)np/64 + 1;
		if((rc = ctx->rp_foot.ensure(nv)) != PCR_OK) return rc;
		if((rc = ctx->rp_keys.ensure(2*(size_t)np + held_words)) != PCR_OK) return rc;
		// uint32 scratch: sites [nv] | var_first [n_ol + 1] | run_first [n_ol + 1] | pair values 2 x [np] | run_sum [np] | run_start [np + 1] |
		// candidates [n_ol x max_candidates] | going [RP_SLOTS]
		const size_t n_cand_all = (size_t)n_ol*max_candidates;
		if((rc = ctx->rp_u32.ensure((size_t)nv + 2*((size_t)n_ol + 1) + 4*(size_t)np + 1 + n_cand_all + RP_SLOTS)) != PCR_OK) return rc;
		if((rc = ctx->rp_state.ensure((size_t)n_ol*sizeof(RpState) + n_cand_all*sizeof(RpScore))) != PCR_OK) return rc;
		if((rc = ctx->rp_rec.ensure((size_t)n_ol*RP_SLOTS)) != PCR_OK) return rc;
		uint4 *const foot = ctx->rp_foot.p;
		uint64_t *const pk0 = ctx->rp_keys.p, *const pk1 = pk0 + np, *const held = pk1 + np;
		uint32_t *const sites = ctx->rp_u32.p, *const var_first = sites + nv, *const run_first = var_first + n_ol + 1;
		uint32_t *const pv0 = run_first + n_ol + 1, *const pv1 = pv0 + np, *const run_sum = pv1 + np, *const run_start = run_sum + np;
		uint32_t *const cand = run_start + np + 1, *const going = cand + n_cand_all;
		RpState *const state = (RpState *)ctx->rp_state.p;
		RpScore *const score = (RpScore *)(ctx->rp_state.p + (size_t)n_ol*sizeof(RpState));
		pcr_repair_step *const d_rec = ctx->rp_rec.p;
		HIP_TRY(hipMemsetAsync(held, 0, held_words*sizeof(uint64_t), ctx->stream));
		HIP_TRY(hipMemsetAsync(going, 0, RP_SLOTS*sizeof(uint32_t), ctx->stream));
		// ---- 1. footprints in record order, the oligos' record ranges
		hipLaunchKernelGGL(k_rp_variants, dim3(grid_v), dim3(POOL_THREADS), 0, ctx->stream, run.sv, run.key_ord, run.start, run.rank, nv, run.d_ol, foot, sites);
		HIP_TRY(hipGetLastError());
		hipLaunchKernelGGL(k_rp_bounds<false>, dim3(grid_o), dim3(POOL_THREADS), 0, ctx->stream, run.rec, (const uint64_t *)nullptr, 0u,
			(const uint32_t *)nullptr, nv, n_ol, var_first);
		HIP_TRY(hipGetLastError());
		// ---- 2. the distinct (variant, sequence) pairs by (oligo, sequence), the sequence runs
		hipLaunchKernelGGL(k_rp_pairs, dim3(grid_i), dim3(POOL_THREADS), 0, ctx->stream, run.sv, run.key_ord, run.sum, run.rank, ni, seq_bits, pk0, pv0);
		HIP_TRY(hipGetLastError());
		size_t t1 = 0, t2 = 0;
		HIP_TRY(rocprim::radix_sort_pairs(nullptr, t1, pk0, pk1, pv0, pv1, np, 0, oligo_bits + seq_bits, ctx->stream));
		HIP_TRY(rocprim::inclusive_scan(nullptr, t2, run_sum, run_sum, (size_t)np, rocprim::plus<uint32_t>(), ctx->stream));
		if((rc = ctx->site_tmp.ensure(std::max(t1, t2) + 16)) != PCR_OK) return rc;
		HIP_TRY(rocprim::radix_sort_pairs(ctx->site_tmp.p, t1, pk0, pk1, pv0, pv1, np, 0, oligo_bits + seq_bits, ctx->stream));
		hipLaunchKernelGGL(k_rp_heads, dim3(grid_p), dim3(POOL_THREADS), 0, ctx->stream, (const uint64_t *)pk1, np, pv0);   // (pv0 is spent)
		HIP_TRY(hipGetLastError());
		HIP_TRY(rocprim::inclusive_scan(ctx->site_tmp.p, t2, pv0, run_sum, (size_t)np, rocprim::plus<uint32_t>(), ctx->stream));
		hipLaunchKernelGGL(k_rp_runs, dim3(grid_p), dim3(POOL_THREADS), 0, ctx->stream, (const uint32_t *)run_sum, np, run_start);
		HIP_TRY(hipGetLastError());
		hipLaunchKernelGGL(k_rp_bounds<true>, dim3(grid_o), dim3(POOL_THREADS), 0, ctx->stream, (const pcr_site_variant *)nullptr, (const uint64_t *)pk1, seq_bits,
			(const uint32_t *)run_sum, np, n_ol, run_first);
		HIP_TRY(hipGetLastError());
		// ---- 3. step 0; 4. the steps, until no oligo goes on
		const RpRule rule = { max_degeneracy, max_mismatch, clamp3, max_candidates, max_steps };
		hipLaunchKernelGGL(k_rp_step<true>, dim3(n_ol), dim3(POOL_THREADS), 0, ctx->stream, run.d_ol, (const uint32_t *)var_first, (const uint4 *)foot,
			(const uint32_t *)sites, (const uint32_t *)run_first, (const uint32_t *)run_start, (const uint32_t *)pv1, held, rule, state,
			(const uint32_t *)cand, (const RpScore *)score, d_rec, going);
		HIP_TRY(hipGetLastError());
		uint32_t n_going = 0;
		HIP_TRY(hipMemcpyAsync(&n_going, going, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
		HIP_TRY(hipStreamSynchronize(ctx->stream));
		for(uint32_t s = 1;s <= max_steps && n_going;++s){
			hipLaunchKernelGGL(k_rp_candidates, dim3(n_ol), dim3(POOL_THREADS), 0, ctx->stream, run.d_ol, (const uint32_t *)var_first, (const uint4 *)foot,
				rule, state, cand);
			HIP_TRY(hipGetLastError());
			hipLaunchKernelGGL(k_rp_weigh, dim3(std::min(max_candidates, nv), n_ol), dim3(POOL_THREADS), 0, ctx->stream, run.d_ol, (const uint32_t *)var_first,
				(const uint4 *)foot, (const uint32_t *)sites, (const uint32_t *)run_first, (const uint32_t *)run_start, (const uint32_t *)pv1,
				(const uint64_t *)held, rule, (const RpState *)state, (const uint32_t *)cand, score);
			HIP_TRY(hipGetLastError());
			hipLaunchKernelGGL(k_rp_step<false>, dim3(n_ol), dim3(POOL_THREADS), 0, ctx->stream, run.d_ol, (const uint32_t *)var_first, (const uint4 *)foot,
				(const uint32_t *)sites, (const uint32_t *)run_first, (const uint32_t *)run_start, (const uint32_t *)pv1, held, rule, state,
				(const uint32_t *)cand, (const RpScore *)score, d_rec, going + s);
			HIP_TRY(hipGetLastError());
			HIP_TRY(hipMemcpyAsync(&n_going, going + s, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
			HIP_TRY(hipStreamSynchronize(ctx->stream));
		}
		// ---- 5. the records: each oligo's steps 0 .. its last
		std::vector<pcr_repair_step> all((size_t)n_ol*RP_SLOTS);
		std::vector<RpState> fin(n_ol);
		HIP_TRY(hipMemcpyAsync(all.data(), d_rec, all.size()*sizeof(pcr_repair_step), hipMemcpyDeviceToHost, ctx->stream));
		HIP_TRY(hipMemcpyAsync(fin.data(), state, fin.size()*sizeof(RpState), hipMemcpyDeviceToHost, ctx->stream));
		HIP_TRY(hipStreamSynchronize(ctx->stream));
		for(uint32_t o = 0;o < n_ol;++o){
			for(uint32_t s = 0;s <= fin[o].step;++s) recs.push_back(all[(size_t)o*RP_SLOTS + s]);
			if(!recs.back().flags){ g_err = "pcr_site_repair: internal error: an oligo's last step carries no reason"; return PCR_ERR_RANGE; }
		}
	}
	const uint64_t n = recs.size();
	if(n > cap) return (int64_t)n;                                               // count only: nothing is melted, out is left as it is
	if(args){
		std::vector<pcr_word128> words(n);
		std::vector<pcr_thermo_result> res(n);
		for(uint64_t i = 0;i < n;++i) words[i] = recs[i].word;
		if((rc = pcr_thermo(ctx, words.data(), (uint32_t)n, check_homo_dimer, args, res.data())) != PCR_OK) return rc;
		for(uint64_t i = 0;i < n;++i) recs[i].valid = res[i].valid;
	}
	memcpy(out, recs.data(), n*sizeof(pcr_repair_step));
	return (int64_t)n;
}

} // extern "C"
