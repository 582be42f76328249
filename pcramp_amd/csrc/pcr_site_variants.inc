// A panel's binding sites grouped by what the template spells there (pcr_site_variants; included by pcr_device.hip after
// pcr_site_tm.inc, whose item kernel, pick rule and melting body it shares).
//
// The sites are pcr_site_tm's.  k_site_tm spells both strands of a site's duplex from the oligo's slot masks and from the
// picked entry's planes inside T = site_window(start, stop), and DB words are oligo-oriented on both strands: every site with
// the same (oligo, planes & T) has bit-identical tm_max, tm_min, dH, dS, matches and flags.  That pair is the key, compared in
// full -- no hash:
//   1. k_pool_entry_oligos<false> / <true> + a scan: the (entry, oligo) items, as pcr_site_tm's step 1.
//   2. k_sv_items: per item the picked entry's planes & T, its oligo, sequence, loc5 and strand (a SvItem).
//   3. Five stable LSD radix sorts of the item order: (loc5, strand), (oligo, sequence) -- pcr_site_tm's record order, kept for
//      the site map -- then (g, t), (a, c), oligo.  Items of a key are now consecutive, in (sequence, loc5, strand) order.
//   4. k_sv_heads + one scan: a position opens a variant where the key changes and a sequence where that or the sequence
//      changes; both flags ride one 64-bit sum.  k_sv_groups: where each variant starts, and every item's variant.  A variant's
//      first member is its first position, its sequences are a difference of the scan's high half.
//   5. k_sv_records: a thread per variant: word, matches, mismatch mask, clamps, flags, counts, the first member.
//   6. With thermodynamics: a scan of n_expansions, k_sv_tm (k_site_tm's loop with site_melt on the variant's planes: one wave
//      per (variant, expansion)), k_sv_reduce (k_site_reduce's rule).
//   7. Two stable sorts of the variants into record order, k_sv_gather, and k_sv_map for the site map.
// Steps 1, 3 and 6 use pcr_site_tm's scratch (pcr_ctx::site_*: nothing is kept in it between calls); the rest is pcr_ctx::sv_*.
// sv_check (the refusals before the handle, the distinct oligos) and sv_run (steps 1 to 7) are shared with pcr_site_repair.inc,
// which goes on from what sv_run leaves on the device (SvRun); pcr_site_variants adds the site map and the copy-out.

namespace {

struct SvItem { Planes w; uint32_t oligo, seq; int32_t loc5; uint32_t strand; };    // w: the picked entry's planes & T

__device__ __forceinline__ bool sv_same_key(const SvItem &x, const SvItem &y)
{
	return x.oligo == y.oligo && x.w.a == y.w.a && x.w.c == y.w.c && x.w.g == y.w.g && x.w.t == y.w.t;
}

__global__ __launch_bounds__(POOL_THREADS) void k_sv_items(const DevEntry *__restrict__ db, uint32_t cap, const uint32_t *__restrict__ touched,
	const uint32_t *__restrict__ seg_hi, const uint2 *__restrict__ items, uint32_t n_items, const PoolOligo *__restrict__ oligos,
	SvItem *__restrict__ sv, uint64_t *__restrict__ key, uint32_t *__restrict__ ord)
{
	const uint32_t k = blockIdx.x*blockDim.x + threadIdx.x;
	if(k >= n_items) return;
	const uint2 it = items[k];
	const PoolOligo o = oligos[it.y];
	const uint32_t slot = site_slot(it.x, cap, touched);
	const uint32_t T = site_window(o.start, o.stop);
	const DevEntry en = site_pick(db, slot, seg_hi[db[slot].seq], o, T);
	SvItem s;
	s.w.a = en.w.a & T; s.w.c = en.w.c & T; s.w.g = en.w.g & T; s.w.t = en.w.t & T;
	s.oligo = it.y; s.seq = en.seq; s.strand = en.strand;
	s.loc5 = (en.strand == 1) ? en.loc + o.start : en.loc - o.stop;              // sequence.h:57-65
	sv[k] = s;
	key[k] = ((uint64_t)((uint32_t)s.loc5 ^ 0x80000000u) << 1) | (en.strand - 1u);   // k_site_key1's
	ord[k] = k;
}

// the key of the next sort pass, of the items in their present order
enum { SV_KEY_OLIGO_SEQ, SV_KEY_GT, SV_KEY_AC, SV_KEY_OLIGO };
template<int WHAT>
__global__ __launch_bounds__(POOL_THREADS) void k_sv_key(const SvItem *__restrict__ sv, const uint32_t *__restrict__ ord, uint32_t n_items,
	uint32_t seq_bits, uint64_t *__restrict__ key)
{
	const uint32_t r = blockIdx.x*blockDim.x + threadIdx.x;
	if(r >= n_items) return;
	const SvItem s = sv[ord[r]];
	if(WHAT == SV_KEY_OLIGO_SEQ) key[r] = ((uint64_t)s.oligo << seq_bits) | s.seq;   // k_site_key2's
	else if(WHAT == SV_KEY_GT) key[r] = ((uint64_t)s.w.g << 32) | s.w.t;
	else if(WHAT == SV_KEY_AC) key[r] = ((uint64_t)s.w.a << 32) | s.w.c;
	else key[r] = s.oligo;
}

// bit 0: position s opens a variant; bit 32: it opens a sequence of its variant
__global__ __launch_bounds__(POOL_THREADS) void k_sv_heads(const SvItem *__restrict__ sv, const uint32_t *__restrict__ ord, uint32_t n_items,
	uint64_t *__restrict__ flag)
{
	const uint32_t s = blockIdx.x*blockDim.x + threadIdx.x;
	if(s >= n_items) return;
	bool head = true, seq_head = true;
	if(s > 0){
		const SvItem x = sv[ord[s]], y = sv[ord[s - 1]];
		head = !sv_same_key(x, y);
		seq_head = head || x.seq != y.seq;
	}
	flag[s] = (head ? 1ull : 0ull) | (seq_head ? 1ull << 32 : 0ull);
}

// sum: the inclusive scan of the flags.  Variant v = (low half) - 1 starts where the low half steps; start[n_var] = n_items.
__global__ __launch_bounds__(POOL_THREADS) void k_sv_groups(const uint32_t *__restrict__ ord, const uint64_t *__restrict__ sum, uint32_t n_items,
	uint32_t n_var, uint32_t *__restrict__ start, uint32_t *__restrict__ item_var)
{
	const uint32_t s = blockIdx.x*blockDim.x + threadIdx.x;
	if(s >= n_items) return;
	const uint32_t v = (uint32_t)sum[s] - 1u;
	item_var[ord[s]] = v;
	if(s == 0 || (uint32_t)sum[s - 1] != (uint32_t)sum[s]) start[v] = s;
	if(s == 0) start[n_var] = n_items;
}

// Variant v in key order: everything but the thermodynamics; its job count and its first record-order sort key.
__global__ __launch_bounds__(POOL_THREADS) void k_sv_records(const SvItem *__restrict__ sv, const uint32_t *__restrict__ ord,
	const uint64_t *__restrict__ sum, const uint32_t *__restrict__ start, uint32_t n_var, const PoolOligo *__restrict__ oligos,
	const SiteOligoX *__restrict__ ox, pcr_site_variant *__restrict__ rec, uint32_t *__restrict__ count, uint64_t *__restrict__ key,
	uint32_t *__restrict__ vord)
{
	const uint32_t v = blockIdx.x*blockDim.x + threadIdx.x;
	if(v >= n_var) return;
	const uint32_t s0 = start[v], s1 = start[v + 1];
	const SvItem it = sv[ord[s0]];                                                // the lowest member in (sequence, loc5, strand)
	const PoolOligo o = oligos[it.oligo];
	pcr_site_variant r;
	r.word.w[0] = r.word.w[1] = 0ull;
	for(uint32_t k = 0;k < 32u;++k){                                              // word.cpp:11-16: slot k is nibble 15 - k % 16 of block k / 16
		const uint64_t nib = ((it.w.a >> k) & 1u) | (((it.w.c >> k) & 1u) << 1) | (((it.w.g >> k) & 1u) << 2) | (((it.w.t >> k) & 1u) << 3);
		r.word.w[k >> 4] |= nib << ((15u - (k & 15u))*4u);
	}
	const uint32_t hit = (it.w.a & o.m.a) | (it.w.c & o.m.c) | (it.w.g & o.m.g) | (it.w.t & o.m.t);
	const uint32_t upto = (o.stop >= 31) ? 0xFFFFFFFFu : ((1u << (o.stop + 1)) - 1u);
	const uint32_t miss = ~hit & upto & ~((1u << o.start) - 1u);                  // the oligo's slots (no hole: the host refuses it) that match nothing
	r.oligo = it.oligo;
	r.sites = s1 - s0;
	r.sequences = (uint32_t)(sum[s1 - 1] >> 32) - (uint32_t)(sum[s0] >> 32) + 1u;
	r.matches = (uint32_t)__popc(hit);
	r.mismatch_mask = miss >> o.start;
	r.clamp3 = miss ? (uint32_t)(o.stop - (31 - (int)__builtin_clz(miss))) : (uint32_t)(o.stop - o.start + 1);
	r.clamp5 = miss ? (uint32_t)((int)__builtin_ctz(miss) - o.start) : (uint32_t)(o.stop - o.start + 1);
	r.n_expansions = ox[it.oligo].n_exp;
	int lo, hi;
	r.flags = site_stretch(it.w, site_window(o.start, o.stop), lo, hi) ? 0u : PCR_SITE_NO_TM;
	r.first_sequence = it.seq; r.first_loc5 = it.loc5; r.first_strand = it.strand;
	r.tm_max = r.tm_min = r.dH = r.dS = 0.0f;
	rec[v] = r;
	count[v] = r.n_expansions;
	key[v] = ((uint64_t)(~r.sites) << 32) | (63u - r.matches);                    // sites descending, then matches descending
	vord[v] = v;
}

// Job j = expansion j - joff[v] of variant v: k_site_tm with the variant's planes for the picked entry's.
__global__ __launch_bounds__(SITE_THREADS) void k_sv_tm(const SvItem *__restrict__ sv, const uint32_t *__restrict__ ord,
	const uint32_t *__restrict__ start, uint32_t n_var, const uint64_t *__restrict__ joff, uint32_t n_jobs,
	const PoolOligo *__restrict__ oligos, const SiteOligoX *__restrict__ ox, const int *__restrict__ dg_global, float log_na, float4 *__restrict__ res)
{
	using namespace thermo;
	extern __shared__ int site_lds[];                                             // dg [49*49] | SITE_WAVES slabs
	const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63u;
	Engine<1> e;
	WaveSlab &w = site_engine(site_lds, dg_global, log_na, wave, e);
	for(unsigned j = blockIdx.x*SITE_WAVES + wave;j < n_jobs;j += gridDim.x*SITE_WAVES){   // uniform per wave
		unsigned v = 0, above = n_var;                                             // joff[v] <= j < joff[above]
		while(above - v > 1u){
			const unsigned mid = v + (above - v)/2u;
			if(joff[mid] <= (uint64_t)j) v = mid; else above = mid;
		}
		const SvItem it = sv[ord[start[v]]];
		const PoolOligo o = oligos[it.oligo];
		float4 r;
		site_melt(e, w, lane, o, ox[it.oligo].log_strand, it.w, site_window(o.start, o.stop), j - (unsigned)joff[v], r);
		if(lane == 0) res[j] = r;
	}
}

// k_site_reduce's rule on variant v: the highest Tm (the lowest expansion on a tie) gives dH and dS.
__global__ __launch_bounds__(POOL_THREADS) void k_sv_reduce(const uint64_t *__restrict__ joff, const float4 *__restrict__ res, uint32_t n_var,
	pcr_site_variant *__restrict__ rec, uint32_t *__restrict__ error)
{
	const uint32_t v = blockIdx.x*blockDim.x + threadIdx.x;
	if(v >= n_var) return;
	const uint64_t j0 = joff[v], j1 = joff[v + 1];
	float tm_max = 0.0f, tm_min = 0.0f, dH = 0.0f, dS = 0.0f;
	uint32_t st = 0;
	for(uint64_t j = j0;j < j1;++j){
		const float4 x = res[j];
		st |= __float_as_uint(x.w);
		if(j == j0 || x.x > tm_max){ tm_max = x.x; dH = x.y; dS = x.z; }
		if(j == j0 || x.x < tm_min) tm_min = x.x;
	}
	if(st & SITE_ST_NO_TM) tm_max = tm_min = dH = dS = 0.0f;
	if(st & SITE_ST_ERROR) atomicOr(error, 1u);
	rec[v].tm_max = tm_max; rec[v].tm_min = tm_min; rec[v].dH = dH; rec[v].dS = dS;
}

// the second record-order key of the variants in their (sites, matches, planes) order: oligo, then sequences descending
__global__ __launch_bounds__(POOL_THREADS) void k_sv_vkey2(const pcr_site_variant *__restrict__ rec, const uint32_t *__restrict__ vord, uint32_t n_var,
	uint64_t *__restrict__ key)
{
	const uint32_t f = blockIdx.x*blockDim.x + threadIdx.x;
	if(f >= n_var) return;
	const pcr_site_variant &r = rec[vord[f]];
	key[f] = ((uint64_t)r.oligo << 32) | (uint32_t)~r.sequences;
}

__global__ __launch_bounds__(POOL_THREADS) void k_sv_gather(const pcr_site_variant *__restrict__ rec, const uint32_t *__restrict__ vord, uint32_t n_var,
	pcr_site_variant *__restrict__ out, uint32_t *__restrict__ rank)
{
	const uint32_t f = blockIdx.x*blockDim.x + threadIdx.x;
	if(f >= n_var) return;
	const uint32_t v = vord[f];
	out[f] = rec[v];
	rank[v] = f;
}

// site r of pcr_site_tm's record order -> the record of its variant
__global__ __launch_bounds__(POOL_THREADS) void k_sv_map(const uint32_t *__restrict__ site_ord, const uint32_t *__restrict__ item_var,
	const uint32_t *__restrict__ rank, uint32_t n_items, uint32_t *__restrict__ map)
{
	const uint32_t r = blockIdx.x*blockDim.x + threadIdx.x;
	if(r < n_items) map[r] = rank[item_var[site_ord[r]]];
}

static_assert(sizeof(pcr_site_variant) == 80, "record layout");
static_assert(sizeof(SvItem) == 32, "item layout");
static_assert(POOL_MAX_OLIGOS <= (1u << 16), "k_sv_vkey2 keeps the oligo above 32 bits of a 48-bit key");

// What one run of the pipeline leaves on the device for its caller (pcr_site_variants copies it out, pcr_site_repair.inc goes
// on from it): valid until the next call that uses pcr_ctx::site_* or sv_*.
struct SvRun {
	bool done = false;                 // the records exist (false: the run ended early with a count, an empty answer or an error)
	uint32_t n_ol = 0, ni = 0, nv = 0, n_vseq = 0;   // distinct oligos, sites, variants, distinct (variant, sequence) pairs
	uint64_t n_jobs = 0;
	const PoolOligo *d_ol = nullptr;
	const SvItem *sv = nullptr;        // the items
	const uint32_t *key_ord = nullptr, *site_ord = nullptr;   // position in key order -> item; pcr_site_tm's record order -> item
	const uint64_t *sum = nullptr;     // k_sv_heads' flags scanned, by position in key order
	const uint32_t *start = nullptr;   // variant (key order) -> its first position; start[nv] = ni
	const uint32_t *item_var = nullptr, *rank = nullptr;      // item -> variant (key order); variant (key order) -> record
	const pcr_site_variant *rec = nullptr;                    // the records in record order
};

// The arguments every caller of the pipeline refuses before the handle (pcr_site_tm's, in its order; args may be NULL), and the
// distinct oligos (site_oligo_table, pcr_site_tm.inc).  bad_out: the caller's own "cap without a buffer".
int sv_check(const char *who, pcr_set which, const pcr_pair *pairs, uint32_t n_pairs, float threshold, const pcr_thermo_args *args,
	float template_strand, uint32_t *oligo_id, bool bad_out, std::vector<PoolOligo> &ol, std::vector<SiteOligoX> &olx)
{
	const std::string w(who);
	if(!set_ok(which)){ g_err = w + ": unknown sequence set"; return PCR_ERR_ARG; }
	if(which != PCR_SET_TARGET && which != PCR_SET_BACKGROUND){ g_err = w + ": PCR_SET_MULTIPLEX is not supported (PCR_SET_TARGET or PCR_SET_BACKGROUND)"; return PCR_ERR_ARG; }
	if((n_pairs && (!pairs || !oligo_id)) || bad_out){ g_err = w + ": bad argument"; return PCR_ERR_ARG; }
	if(n_pairs > PCR_POOL_MAX_PAIRS){ g_err = w + ": panel larger than PCR_POOL_MAX_PAIRS"; return PCR_ERR_ARG; }
	if(args){
		if(!(template_strand >= 0.0f) || !(args->primer_strand >= 0.0f)){ g_err = w + ": negative strand concentration (NucCruc::strand, nuc_cruc.h:818-826)"; return PCR_ERR_ARG; }
		if(!(args->salt >= 1.0e-6f && args->salt <= 1.0f)){ g_err = w + ": salt outside [1e-6, 1] (NucCruc::salt, nuc_cruc.h:780-788)"; return PCR_ERR_ARG; }
	}
	return site_oligo_table(w, "an oligo", "primer_strand", pairs, n_pairs, threshold, args, template_strand, oligo_id, ol, olx);
}

// Steps 1 to 7 on a checked panel -> the number of variants or a negative error; `run` says what is where.  A count above cap
// ends the run before the records (no thermodynamics, run.done stays false) unless always is set.
int64_t sv_run(const char *who, pcr_ctx *ctx, pcr_set which, uint32_t n_pairs, const pcr_thermo_args *args, const std::vector<PoolOligo> &ol,
	const std::vector<SiteOligoX> &olx, uint64_t cap, bool always, uint64_t counts[2], SvRun &run)
{
	const std::string w(who);
	if(!ctx){ g_err = w + ": null handle"; return PCR_ERR_ARG; }
	{ const int drc = drain(ctx); if(drc != PCR_OK) return drc; }
	HIP_TRY(hipSetDevice(ctx->device));
	SeqSet &S = ctx->sets[which];
	if(!S.have_db){ g_err = w + ": no word DB (call pcr_select_words or pcr_select_sites first)"; return PCR_ERR_STATE; }
	if(counts) counts[0] = counts[1] = 0;
	if(n_pairs == 0) return 0;
	{ const int erc = ensure_touched(ctx, S); if(erc != PCR_OK) return erc; }
	if(S.n_entries == 0 || S.n_touched == 0) return 0;
	const uint32_t n_ol = (uint32_t)ol.size();
	int rc;
	const size_t ol_bytes = ol.size()*sizeof(PoolOligo), olx_bytes = olx.size()*sizeof(SiteOligoX);
	if((rc = ctx->site_in.ensure(ol_bytes + olx_bytes)) != PCR_OK) return rc;
	const PoolOligo *d_ol = (const PoolOligo *)ctx->site_in.p;
	const SiteOligoX *d_olx = (const SiteOligoX *)(ctx->site_in.p + ol_bytes);
	HIP_TRY(hipMemcpyAsync(ctx->site_in.p, ol.data(), ol_bytes, hipMemcpyHostToDevice, ctx->stream));
	HIP_TRY(hipMemcpyAsync(ctx->site_in.p + ol_bytes, olx.data(), olx_bytes, hipMemcpyHostToDevice, ctx->stream));
	// ---- 1. the items (item_count, item_fill)
	const ItemBufs B{&ctx->site_tmp, &ctx->site_cnt, &ctx->site_eoff, &ctx->site_items};
	uint64_t n_items = 0;
	if((rc = item_count(ctx, S, d_ol, n_ol, B, n_items)) != PCR_OK) return rc;
	if(n_items >= POOL_MAX_ITEMS){ g_err = w + ": too many sites"; return PCR_ERR_CAPACITY; }
	if(counts) counts[0] = n_items;
	if(n_items == 0) return 0;
	if((rc = item_fill(ctx, S, d_ol, n_ol, B, n_items)) != PCR_OK) return rc;
	// ---- 2. what each item spells; 3. the orders
	const uint32_t ni = (uint32_t)n_items;
	const unsigned grid_i = (ni + POOL_THREADS - 1)/POOL_THREADS;
	if((rc = ctx->sv_item.ensure((size_t)ni*sizeof(SvItem))) != PCR_OK) return rc;
	if((rc = ctx->site_keys.ensure(2*(size_t)ni)) != PCR_OK) return rc;
	if((rc = ctx->site_ord.ensure(2*(size_t)ni)) != PCR_OK) return rc;
	if((rc = ctx->sv_ord.ensure(2*(size_t)ni)) != PCR_OK) return rc;
	SvItem *const sv_w = (SvItem *)ctx->sv_item.p;
	const SvItem *sv = sv_w;
	uint64_t *k0 = ctx->site_keys.p, *k1 = k0 + ni;
	uint32_t *o0 = ctx->site_ord.p, *o1 = o0 + ni;                               // o0 ends as pcr_site_tm's record order and is kept
	uint32_t *g0 = ctx->sv_ord.p, *g1 = g0 + ni;                                 // g0 ends as the key order
	hipLaunchKernelGGL(k_sv_items, dim3(grid_i), dim3(POOL_THREADS), 0, ctx->stream, S.db.p, S.db_cap, S.touched.p, S.d_seg_hi,
		(const uint2 *)ctx->site_items.p, ni, d_ol, sv_w, k0, o0);
	HIP_TRY(hipGetLastError());
	const unsigned seq_bits = pool_bits(S.n), oligo_bits = pool_bits(n_ol);
	size_t t1 = 0, t2 = 0, t3 = 0, t4 = 0;
	HIP_TRY(rocprim::radix_sort_pairs(nullptr, t1, k0, k1, o0, o1, ni, 0, 33, ctx->stream));
	HIP_TRY(rocprim::radix_sort_pairs(nullptr, t2, k0, k1, o1, o0, ni, 0, oligo_bits + seq_bits, ctx->stream));
	HIP_TRY(rocprim::radix_sort_pairs(nullptr, t3, k0, k1, o0, g0, ni, 0, 64, ctx->stream));
	HIP_TRY(rocprim::radix_sort_pairs(nullptr, t4, k0, k1, g1, g0, ni, 0, oligo_bits, ctx->stream));
	const size_t sort_tmp = std::max(std::max(t1, t2), std::max(t3, t4));
	if((rc = ctx->site_tmp.ensure(sort_tmp + 16)) != PCR_OK) return rc;
	HIP_TRY(rocprim::radix_sort_pairs(ctx->site_tmp.p, t1, k0, k1, o0, o1, ni, 0, 33, ctx->stream));
	hipLaunchKernelGGL(k_sv_key<SV_KEY_OLIGO_SEQ>, dim3(grid_i), dim3(POOL_THREADS), 0, ctx->stream, sv, (const uint32_t *)o1, ni, seq_bits, k0);
	HIP_TRY(hipGetLastError());
	HIP_TRY(rocprim::radix_sort_pairs(ctx->site_tmp.p, t2, k0, k1, o1, o0, ni, 0, oligo_bits + seq_bits, ctx->stream));   // (stable, as every pass below)
	hipLaunchKernelGGL(k_sv_key<SV_KEY_GT>, dim3(grid_i), dim3(POOL_THREADS), 0, ctx->stream, sv, (const uint32_t *)o0, ni, seq_bits, k0);
	HIP_TRY(hipGetLastError());
	HIP_TRY(rocprim::radix_sort_pairs(ctx->site_tmp.p, t3, k0, k1, o0, g0, ni, 0, 64, ctx->stream));
	hipLaunchKernelGGL(k_sv_key<SV_KEY_AC>, dim3(grid_i), dim3(POOL_THREADS), 0, ctx->stream, sv, (const uint32_t *)g0, ni, seq_bits, k0);
	HIP_TRY(hipGetLastError());
	HIP_TRY(rocprim::radix_sort_pairs(ctx->site_tmp.p, t3, k0, k1, g0, g1, ni, 0, 64, ctx->stream));
	hipLaunchKernelGGL(k_sv_key<SV_KEY_OLIGO>, dim3(grid_i), dim3(POOL_THREADS), 0, ctx->stream, sv, (const uint32_t *)g1, ni, seq_bits, k0);
	HIP_TRY(hipGetLastError());
	HIP_TRY(rocprim::radix_sort_pairs(ctx->site_tmp.p, t4, k0, k1, g1, g0, ni, 0, oligo_bits, ctx->stream));
	// ---- 4. the variants: heads, their scan, starts
	hipLaunchKernelGGL(k_sv_heads, dim3(grid_i), dim3(POOL_THREADS), 0, ctx->stream, sv, (const uint32_t *)g0, ni, k0);
	HIP_TRY(hipGetLastError());
	size_t tmp = 0;
	HIP_TRY(rocprim::inclusive_scan(nullptr, tmp, k0, k1, (size_t)ni, rocprim::plus<uint64_t>(), ctx->stream));
	if((rc = ctx->site_tmp.ensure(tmp + 16)) != PCR_OK) return rc;
	HIP_TRY(rocprim::inclusive_scan(ctx->site_tmp.p, tmp, k0, k1, (size_t)ni, rocprim::plus<uint64_t>(), ctx->stream));
	uint64_t last = 0;
	HIP_TRY(hipMemcpyAsync(&last, k1 + (ni - 1), sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
	HIP_TRY(hipStreamSynchronize(ctx->stream));
	const uint32_t nv = (uint32_t)last;                                          // 1 .. ni
	run.n_ol = n_ol; run.ni = ni; run.nv = nv; run.n_vseq = (uint32_t)(last >> 32);
	if(!always && nv > cap) return (int64_t)nv;                                  // count only: the caller leaves out and site_variant as they are
	if((rc = ctx->sv_start.ensure((size_t)nv + 1)) != PCR_OK) return rc;
	if((rc = ctx->sv_var.ensure(ni)) != PCR_OK) return rc;
	hipLaunchKernelGGL(k_sv_groups, dim3(grid_i), dim3(POOL_THREADS), 0, ctx->stream, (const uint32_t *)g0, (const uint64_t *)k1, ni, nv,
		ctx->sv_start.p, ctx->sv_var.p);
	HIP_TRY(hipGetLastError());
	// ---- 5. the records in key order
	const unsigned grid_v = (nv + POOL_THREADS - 1)/POOL_THREADS;
	if((rc = ctx->sv_rec.ensure(2*(size_t)nv)) != PCR_OK) return rc;
	if((rc = ctx->sv_vkeys.ensure(2*(size_t)nv)) != PCR_OK) return rc;
	if((rc = ctx->sv_vord.ensure(3*(size_t)nv)) != PCR_OK) return rc;
	if((rc = ctx->site_cnt.ensure((size_t)nv + 1)) != PCR_OK) return rc;        // (the entry counts are spent)
	if((rc = ctx->site_flag.ensure(1)) != PCR_OK) return rc;
	HIP_TRY(hipMemsetAsync(ctx->site_flag.p, 0, sizeof(uint32_t), ctx->stream));
	pcr_site_variant *r0 = ctx->sv_rec.p, *r1 = r0 + nv;
	uint64_t *vk0 = ctx->sv_vkeys.p, *vk1 = vk0 + nv;
	uint32_t *vo0 = ctx->sv_vord.p, *vo1 = vo0 + nv, *rank = vo1 + nv;
	hipLaunchKernelGGL(k_sv_records, dim3(grid_v), dim3(POOL_THREADS), 0, ctx->stream, sv, (const uint32_t *)g0, (const uint64_t *)k1,
		(const uint32_t *)ctx->sv_start.p, nv, d_ol, d_olx, r0, ctx->site_cnt.p, vk0, vo0);
	HIP_TRY(hipGetLastError());
	// ---- 6. one job per (variant, expansion)
	if(args){
		uint64_t n_jobs64 = 0;
		if((rc = scan_total(ctx, ctx->site_cnt.p, ctx->site_joff, ctx->site_tmp, nv, n_jobs64)) != PCR_OK) return rc;
		if(n_jobs64 >= POOL_MAX_ITEMS){ g_err = w + ": too many (variant, expansion) jobs"; return PCR_ERR_CAPACITY; }
		const uint32_t n_jobs = (uint32_t)n_jobs64;
		if((rc = ensure_dg_table(ctx, args->salt)) != PCR_OK) return rc;
		if(!ctx->sv_attr_set){
			HIP_TRY(hipFuncSetAttribute((const void *)k_sv_tm, hipFuncAttributeMaxDynamicSharedMemorySize, (int)SITE_LDS));
			ctx->sv_attr_set = true;
		}
		if((rc = ctx->site_res.ensure(n_jobs)) != PCR_OK) return rc;
		// at most one block per CU (a block takes most of a CU's LDS), the waves striding over the jobs
		const unsigned grid_j = std::max(1u, std::min<unsigned>((n_jobs + SITE_WAVES - 1)/SITE_WAVES, (unsigned)ctx->n_cu));
		hipLaunchKernelGGL(k_sv_tm, dim3(grid_j), dim3(SITE_THREADS), SITE_LDS, ctx->stream, sv, (const uint32_t *)g0, (const uint32_t *)ctx->sv_start.p, nv,
			(const uint64_t *)ctx->site_joff.p, n_jobs, d_ol, d_olx, (const int *)ctx->th_dg.p, logf(args->salt), ctx->site_res.p);
		HIP_TRY(hipGetLastError());
		hipLaunchKernelGGL(k_sv_reduce, dim3(grid_v), dim3(POOL_THREADS), 0, ctx->stream, (const uint64_t *)ctx->site_joff.p, (const float4 *)ctx->site_res.p, nv,
			r0, ctx->site_flag.p);
		HIP_TRY(hipGetLastError());
		if(counts) counts[1] = n_jobs64;
	}
	// ---- 7. record order: (sites, matches) descending under the planes order the variants are in, then (oligo, sequences descending)
	t1 = t2 = 0;
	HIP_TRY(rocprim::radix_sort_pairs(nullptr, t1, vk0, vk1, vo0, vo1, nv, 0, 64, ctx->stream));
	HIP_TRY(rocprim::radix_sort_pairs(nullptr, t2, vk0, vk1, vo1, vo0, nv, 0, 48, ctx->stream));
	if((rc = ctx->site_tmp.ensure(std::max(t1, t2) + 16)) != PCR_OK) return rc;
	HIP_TRY(rocprim::radix_sort_pairs(ctx->site_tmp.p, t1, vk0, vk1, vo0, vo1, nv, 0, 64, ctx->stream));
	hipLaunchKernelGGL(k_sv_vkey2, dim3(grid_v), dim3(POOL_THREADS), 0, ctx->stream, (const pcr_site_variant *)r0, (const uint32_t *)vo1, nv, vk0);
	HIP_TRY(hipGetLastError());
	HIP_TRY(rocprim::radix_sort_pairs(ctx->site_tmp.p, t2, vk0, vk1, vo1, vo0, nv, 0, 48, ctx->stream));
	hipLaunchKernelGGL(k_sv_gather, dim3(grid_v), dim3(POOL_THREADS), 0, ctx->stream, (const pcr_site_variant *)r0, (const uint32_t *)vo0, nv, r1, rank);
	HIP_TRY(hipGetLastError());
	run.d_ol = d_ol; run.sv = sv; run.key_ord = g0; run.site_ord = o0; run.sum = k1; run.start = ctx->sv_start.p; run.item_var = ctx->sv_var.p;
	run.rank = rank; run.rec = r1; run.done = true;
	return (int64_t)nv;
}

} // namespace

extern "C" {

int64_t pcr_site_variants(pcr_ctx *ctx, pcr_set which, const pcr_pair *pairs, uint32_t n_pairs, float threshold,
	const pcr_thermo_args *args, float template_strand, uint32_t *oligo_id, pcr_site_variant *out, uint64_t cap,
	uint32_t *site_variant, uint64_t site_cap, uint64_t counts[2])
{
	std::vector<PoolOligo> ol;
	std::vector<SiteOligoX> olx;
	int rc = sv_check("pcr_site_variants", which, pairs, n_pairs, threshold, args, template_strand, oligo_id, cap && !out, ol, olx);
	if(rc != PCR_OK) return rc;
	if(site_cap && !site_variant){ g_err = "pcr_site_variants: site_cap without a site_variant buffer"; return PCR_ERR_ARG; }
	SvRun run;
	const int64_t n = sv_run("pcr_site_variants", ctx, which, n_pairs, args, ol, olx, cap, false, counts, run);
	if(!run.done) return n;
	const uint32_t ni = run.ni, nv = run.nv;
	const uint64_t n_items = ni;
	const unsigned grid_i = (ni + POOL_THREADS - 1)/POOL_THREADS;
	const uint32_t *o0 = run.site_ord, *rank = run.rank;
	const pcr_site_variant *r1 = run.rec;
	const bool want_map = site_variant && n_items <= site_cap;
	if(want_map){
		if((rc = ctx->sv_map.ensure(ni)) != PCR_OK) return rc;
		hipLaunchKernelGGL(k_sv_map, dim3(grid_i), dim3(POOL_THREADS), 0, ctx->stream, (const uint32_t *)o0, (const uint32_t *)ctx->sv_var.p,
			(const uint32_t *)rank, ni, ctx->sv_map.p);
		HIP_TRY(hipGetLastError());
		HIP_TRY(hipMemcpyAsync(site_variant, ctx->sv_map.p, (size_t)ni*sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
	}
	uint32_t bad = 0;
	HIP_TRY(hipMemcpyAsync(out, r1, (size_t)nv*sizeof(pcr_site_variant), hipMemcpyDeviceToHost, ctx->stream));
	HIP_TRY(hipMemcpyAsync(&bad, ctx->site_flag.p, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
	HIP_TRY(hipStreamSynchronize(ctx->stream));
	if(bad & 1u){ g_err = "pcr_site_variants: internal trace-back error"; return PCR_ERR_RANGE; }
	return (int64_t)nv;
}

} // extern "C"
