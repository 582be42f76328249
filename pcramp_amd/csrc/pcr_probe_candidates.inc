// Probes proposed from the inserts of a set of products: per assay the oligos most of its sequences hold between the primers
// (pcr_pool_probe_candidates; included by pcr_device.hip after pcr_pool_amplicons.inc).
//
// The host turns each participating record into its insert {sequence, start, length, group} (product_interval: no kernel is handed an
// interval it has not seen pass), adds up the windows, and numbers the START POSITIONS of all inserts consecutively (pos_off[]:
// record k owns max(0, insert - len_min + 1) of them).  From there:
//   1. k_pc_enumerate, a LANE per start position (not a wave or a lane group per record: inserts are 1 to 6 blocks of 32 bases, and
//      every start is the same work).  The lane finds its record by bisection of pos_off[], loads one 32-base plane window
//      (amp_window) and takes from it the length of the A/C/G/T-only prefix, the C and G planes and the shortest length that
//      holds a run longer than max_run: every L of the window is then a few popcounts, for both strands.  A word is its 2-bit codes
//      (A C G T = 0 1 2 3), first base most significant: the forward spelling is a prefix of the interleaved bit-reversed window, the
//      reverse complement a suffix of the complemented one.  The kernel runs twice: counting (a sum per 256 positions), then,
//      after a scan, emitting to exact offsets -- the list is in (record, start, L, strand) order whatever the schedule.
//   2. Three stable radix sorts of an index, least significant key first: the sequence, the spelling, (group, L); what the
//      emission order leaves inside equal keys is (record, start, strand).  k_pc_flags marks the head of every run of one (group, L,
//      word) and the changes of sequence and of record inside it; two scans number the runs and count the changes, so a run's
//      `sequences` and `records` are differences of the scan at its two ends (k_pc_run_keep).
//   3. The runs with sequences >= min_sequences become candidate records (k_pc_cand).  With args: k_pc_jobs writes one
//      thermo::Job each, launch_thermo melts them as it does pcr_thermo's (the homodimer halves mirrored), k_pc_verdict applies
//      thermo_expansion_valid and takes the floats.
//   4. Two more stable sorts, by records and by (group, sequences) -- the candidates are in (group, L, text) order already --,
//      a max-scan for each position's group start, the cut at per_group, a scan, and k_pc_write gathers the kept records.
// Integer work only outside the engine; no atomics except the error flag.  The call owns its scratch (pcr_ctx::ppc_*): 52 bytes
// per occurrence that passes the rules, which the 2^28 limit on the windows bounds.

#include <rocprim/block/block_scan.hpp>
#include <rocprim/block/block_reduce.hpp>

namespace {

constexpr uint32_t PC_THREADS = 256;
constexpr uint32_t PC_BLOCKS_PER_CU = 8;                                        // 8 blocks of 4 waves: the 32 wave slots of a CU; a larger grid would only queue, so the blocks stride
constexpr uint64_t PC_MAX_WINDOWS = 1ull << 28;
constexpr uint32_t PC_DROPPED = PCR_POOL_MAX_PAIRS;                             // the group key of a candidate the engine refused: behind every group

// Waits for the stream when it goes out of scope while armed: declared after the host buffers an asynchronous copy reads, so that an
// early return cannot free them under a pending copy.
struct PcFence { hipStream_t s; bool armed = true; ~PcFence() { if(armed) (void)hipStreamSynchronize(s); } };

struct ProbeRules { uint32_t len_min, len_max, strands, rules, max_run; float gc_min, gc_max; };

// bit i of v -> bit 2i
__device__ __forceinline__ uint64_t pc_spread(uint32_t v32)
{
	uint64_t v = v32;
	v = (v | (v << 16)) & 0x0000FFFF0000FFFFull; v = (v | (v << 8)) & 0x00FF00FF00FF00FFull; v = (v | (v << 4)) & 0x0F0F0F0F0F0F0F0Full;
	v = (v | (v << 2)) & 0x3333333333333333ull; v = (v | (v << 1)) & 0x5555555555555555ull;
	return v;
}

// What start position p gives: its record, where it is, the lengths L (bit L - 1) that pass on strand 1 and on strand 2, and the two
// 64-bit texts every spelling is cut from.
struct PcWindow { uint32_t rec, pos, group, pass1, pass2; uint64_t fwd, rc; };

__device__ __forceinline__ PcWindow pc_window(const uint4 *__restrict__ planes, const uint64_t *__restrict__ blk_off, const uint4 *__restrict__ iv,
	const uint32_t *__restrict__ pos_off, uint32_t n, uint32_t p, const ProbeRules R)
{
	uint32_t k = 0, above = n;                                                    // pos_off[k] <= p < pos_off[above]
	while(above - k > 1u){
		const uint32_t mid = k + (above - k)/2u;
		if(pos_off[mid] <= p) k = mid; else above = mid;
	}
	const uint4 r = iv[k];
	const uint32_t off = p - pos_off[k], left = r.z - off, m = (left < 32u) ? left : 32u;   // left >= len_min: the start is one of the record's
	const uint4 w = amp_window(planes, blk_off[r.x], r.y + off, m);               // (A, C, G, T planes; the bits from m on are clear)
	const uint32_t pairs = (w.x & w.y) | ((w.x | w.y) & (w.z | w.w)) | (w.z & w.w);
	const uint32_t one = (w.x ^ w.y ^ w.z ^ w.w) & ~pairs;                         // exactly A, C, G or T
	const uint32_t prefix = (one == 0xFFFFFFFFu) ? 32u : (uint32_t)__builtin_ctz(~one);   // (<= m)
	// the shortest L whose first L bases hold a run of max_run + 1: bit i of t = bases i .. i + max_run are equal
	uint32_t first_bad = 33u;
	if(R.max_run >= 1u && R.max_run < 32u){
		uint32_t t = ~((w.x ^ (w.x >> 1)) | (w.y ^ (w.y >> 1)) | (w.z ^ (w.z >> 1)) | (w.w ^ (w.w >> 1))) & 0x7FFFFFFFu;
		for(uint32_t i = 1;i < R.max_run;++i) t &= t >> 1;
		if(t) first_bad = (uint32_t)__builtin_ctz(t) + R.max_run + 1u;
	}
	PcWindow W;
	W.rec = k; W.pos = r.y + off; W.group = r.w; W.pass1 = W.pass2 = 0u;
	const uint32_t top = min(min(R.len_max, prefix), first_bad - 1u);
	for(uint32_t L = R.len_min;L <= top;++L){
		const uint32_t mask = (L >= 32u) ? 0xFFFFFFFFu : ((1u << L) - 1u);
		const uint32_t c = __popc(w.y & mask), g = __popc(w.z & mask);
		const float frac = __fdiv_rn((float)(c + g), (float)L);
		if(!(frac >= R.gc_min && frac <= R.gc_max)) continue;
		const bool five_g1 = (w.z & 1u) != 0, five_g2 = ((w.y >> (L - 1u)) & 1u) != 0;   // the reverse complement starts with the complement of base L - 1
		if((R.strands & 1u) && !((R.rules & PCR_PROBE_NO_5G) && five_g1) && !((R.rules & PCR_PROBE_C_GE_G) && c < g)) W.pass1 |= 1u << (L - 1u);
		if((R.strands & 2u) && !((R.rules & PCR_PROBE_NO_5G) && five_g2) && !((R.rules & PCR_PROBE_C_GE_G) && g < c)) W.pass2 |= 1u << (L - 1u);
	}
	const uint32_t lo = w.y | w.w, hi = w.z | w.w;                                 // the 2-bit code of base i: A 0, C 1, G 2, T 3
	W.fwd = pc_spread(__brev(lo)) | (pc_spread(__brev(hi)) << 1);                 // base 0 in bits 63:62: the first L bases are the top 2L bits
	W.rc = pc_spread(~lo) | (pc_spread(~hi) << 1);                                // complemented, base i in bits 2i + 1 : 2i: the low 2L bits read 5' -> 3'
	return W;
}

// A block per chunk of PC_THREADS start positions (the grid strides over the chunks).  EMIT = false: chunk_cnt[chunk] = the
// occurrences of the chunk.  EMIT = true: chunk_off[] is the exclusive scan of those; occurrence i of the whole list gets
// spell[i], rec[i], pos[i] and gls[i] = group << 7 | (L - 1) << 2 | strand.
template<bool EMIT> __global__ __launch_bounds__(PC_THREADS) void k_pc_enumerate(const uint4 *__restrict__ planes, const uint64_t *__restrict__ blk_off,
	const uint4 *__restrict__ iv, const uint32_t *__restrict__ pos_off, uint32_t n, uint32_t n_pos, uint32_t n_chunks, const ProbeRules R,
	uint32_t *__restrict__ chunk_cnt, const uint32_t *__restrict__ chunk_off, uint32_t n_occ, uint64_t *__restrict__ spell, uint32_t *__restrict__ rec,
	uint32_t *__restrict__ pos, uint32_t *__restrict__ gls)
{
	using Scan = rocprim::block_scan<uint32_t, PC_THREADS>;
	using Reduce = rocprim::block_reduce<uint32_t, PC_THREADS>;
	__shared__ typename Scan::storage_type lds_scan;
	__shared__ typename Reduce::storage_type lds_reduce;
	for(uint32_t chunk = blockIdx.x;chunk < n_chunks;chunk += gridDim.x){           // uniform per block
		const uint32_t p = chunk*PC_THREADS + threadIdx.x;
		PcWindow W; W.pass1 = W.pass2 = 0u;
		if(p < n_pos) W = pc_window(planes, blk_off, iv, pos_off, n, p, R);
		const uint32_t cnt = __popc(W.pass1) + __popc(W.pass2);
		if(!EMIT){
			uint32_t total = 0;
			Reduce().reduce(cnt, total, lds_reduce);
			if(threadIdx.x == 0) chunk_cnt[chunk] = total;
		}
		else{
			uint32_t at = 0;
			Scan().exclusive_scan(cnt, at, 0u, lds_scan);
			at += chunk_off[chunk];
			for(uint32_t both = W.pass1 | W.pass2;both;both &= both - 1u){          // L ascending, strand 1 before strand 2
				const uint32_t b = (uint32_t)__builtin_ctz(both), L = b + 1u;
				for(uint32_t strand = 1;strand <= 2u;++strand){
					if(!(((strand == 1u) ? W.pass1 : W.pass2) >> b & 1u)) continue;
					if(at < n_occ){
						spell[at] = (strand == 1u) ? (W.fwd >> (64u - 2u*L)) : ((L >= 32u) ? W.rc : (W.rc & ((1ull << (2u*L)) - 1ull)));
						rec[at] = W.rec; pos[at] = W.pos; gls[at] = (W.group << 7) | (b << 2) | strand;
					}
					++at;
				}
			}
		}
		__syncthreads();                                                            // the next chunk reuses the scan's LDS
	}
}

// key[i] = the sequence of occurrence i, ord[i] = i
__global__ void k_pc_key_seq(const uint4 *__restrict__ iv, const uint32_t *__restrict__ rec, uint32_t n, uint32_t *__restrict__ key, uint32_t *__restrict__ ord)
{
	const uint32_t i = blockIdx.x*blockDim.x + threadIdx.x;
	if(i < n){ key[i] = iv[rec[i]].x; ord[i] = i; }
}

__global__ void k_pc_key_spell(const uint64_t *__restrict__ spell, const uint32_t *__restrict__ ord, uint32_t n, uint64_t *__restrict__ key)
{
	const uint32_t i = blockIdx.x*blockDim.x + threadIdx.x;
	if(i < n) key[i] = spell[ord[i]];
}

__global__ void k_pc_key_gl(const uint32_t *__restrict__ gls, const uint32_t *__restrict__ ord, uint32_t n, uint32_t *__restrict__ key)
{
	const uint32_t i = blockIdx.x*blockDim.x + threadIdx.x;
	if(i < n) key[i] = gls[ord[i]] >> 2;
}

// Sorted position i (0 .. n; position n closes the scans): head[i] = it starts a run of one (group, L, spelling), chg[i] = (the
// sequence changes or a run starts) | (the record changes or a run starts) << 32.
__global__ void k_pc_flags(const uint4 *__restrict__ iv, const uint64_t *__restrict__ spell, const uint32_t *__restrict__ rec, const uint32_t *__restrict__ gls,
	const uint32_t *__restrict__ ord, uint32_t n, uint32_t *__restrict__ head, uint64_t *__restrict__ chg)
{
	const uint32_t i = blockIdx.x*blockDim.x + threadIdx.x;
	if(i > n) return;
	if(i == n){ head[i] = 0u; chg[i] = 0ull; return; }
	const uint32_t o = ord[i];
	bool h = true, s = true, r = true;
	if(i > 0){
		const uint32_t q = ord[i - 1];
		h = (gls[o] >> 2) != (gls[q] >> 2) || spell[o] != spell[q];
		r = h || rec[o] != rec[q];
		s = h || iv[rec[o]].x != iv[rec[q]].x;
	}
	head[i] = h ? 1u : 0u;
	chg[i] = (s ? 1ull : 0ull) | (r ? (1ull << 32) : 0ull);
}

// run_start[run] = the sorted position of its head; run_start[number of runs] = n
__global__ void k_pc_run_start(const uint32_t *__restrict__ head, const uint32_t *__restrict__ run_id, uint32_t n, uint32_t *__restrict__ run_start)
{
	const uint32_t i = blockIdx.x*blockDim.x + threadIdx.x;
	if(i <= n && (i == n || head[i])) run_start[run_id[i]] = i;
}

// keep[run] = its distinct sequences reach min_sequences (keep[n_runs] = 0 closes the scan)
__global__ void k_pc_run_keep(const uint32_t *__restrict__ run_start, const uint64_t *__restrict__ chg_scan, uint32_t n_runs, uint32_t min_sequences,
	uint32_t *__restrict__ keep)
{
	const uint32_t r = blockIdx.x*blockDim.x + threadIdx.x;
	if(r > n_runs) return;
	if(r == n_runs){ keep[r] = 0u; return; }
	const uint32_t sequences = (uint32_t)chg_scan[run_start[r + 1]] - (uint32_t)chg_scan[run_start[r]];
	keep[r] = (sequences >= min_sequences) ? 1u : 0u;
}

// the word of a spelling of L bases, centred as words.centered_word stores an oligo, and its C + G
__device__ __forceinline__ void pc_word(uint64_t spell, uint32_t L, pcr_word128 &word, uint32_t &gc)
{
	word.w[0] = word.w[1] = 0ull; gc = 0u;
	const uint32_t start = (33u - L)/2u;
	for(uint32_t i = 0;i < L;++i){
		const uint32_t code = (uint32_t)(spell >> (2u*(L - 1u - i))) & 3u, slot = start + i;
		word.w[slot >> 4] |= (uint64_t)(1u << code) << ((15u - (slot & 15u))*4u);
		gc += (code == 1u || code == 2u) ? 1u : 0u;
	}
}

// Kept run r -> candidate keep_scan[r]: its record from the run's head (the floats 0) and its spelling.
__global__ void k_pc_cand(const uint32_t *__restrict__ keep, const uint32_t *__restrict__ keep_scan, const uint32_t *__restrict__ run_start,
	const uint64_t *__restrict__ chg_scan, const uint32_t *__restrict__ ord, const uint64_t *__restrict__ spell, const uint32_t *__restrict__ rec,
	const uint32_t *__restrict__ pos, const uint32_t *__restrict__ gls, uint32_t n_runs, pcr_probe_candidate *__restrict__ cand, uint64_t *__restrict__ cand_spell)
{
	const uint32_t r = blockIdx.x*blockDim.x + threadIdx.x;
	if(r >= n_runs || !keep[r]) return;
	const uint32_t c = keep_scan[r], h = run_start[r], o = ord[h];
	const uint64_t a = chg_scan[h], b = chg_scan[run_start[r + 1]];
	const uint32_t g = gls[o];
	pcr_probe_candidate x;
	x.group = g >> 7; x.length = ((g >> 2) & 31u) + 1u;
	pc_word(spell[o], x.length, x.word, x.gc);
	x.sequences = (uint32_t)b - (uint32_t)a; x.records = (uint32_t)(b >> 32) - (uint32_t)(a >> 32);
	x.first_record = rec[o]; x.first_loc5 = (int32_t)pos[o]; x.first_strand = g & 3u;
	x.tm = x.hairpin_tm = x.homodimer_tm = x.dG = 0.0f;
	cand[c] = x;
	cand_spell[c] = spell[o];
}

// one oligo job per candidate: plain codes, as pcr_thermo's jobs arrive in the engine
__global__ void k_pc_jobs(const pcr_probe_candidate *__restrict__ cand, const uint64_t *__restrict__ cand_spell, uint32_t n, int check_homo, float log_strand,
	thermo::Job *__restrict__ jobs)
{
	const uint32_t c = blockIdx.x*blockDim.x + threadIdx.x;
	if(c >= n) return;
	const uint32_t L = cand[c].length;
	const uint64_t s = cand_spell[c];
	thermo::Job j;
	for(uint32_t i = 0;i < (uint32_t)thermo::MAXL;++i){ j.q[i] = (i < L) ? (unsigned char)((s >> (2u*(L - 1u - i))) & 3u) : (unsigned char)0; j.t[i] = 0; }
	j.qlen = (unsigned char)L; j.tlen = 0; j.mode = 0; j.check_homo = check_homo ? 1 : 0;
	j.log_strand = log_strand;
	jobs[c] = j;
}

// pcr_thermo's verdict and floats for candidate c from the engine's results (res[n + c] holds the mirrored homodimer half when
// check_homo); ok[c] = valid.  *flag |= 1 on an internal error of the engine.
__global__ void k_pc_verdict(const thermo::JobOut *__restrict__ res, uint32_t n, int check_homo, const pcr_thermo_args a, pcr_probe_candidate *__restrict__ cand,
	uint32_t *__restrict__ ok, uint32_t *__restrict__ flag)
{
	const uint32_t c = blockIdx.x*blockDim.x + threadIdx.x;
	if(c >= n) return;
	thermo::JobOut o = res[c];
	uint32_t status = o.status;
	if(check_homo){ o.tm_dimer = res[n + c].tm_dimer; status |= res[n + c].status; }
	if(status & 1u) atomicOr(flag, 1u);
	cand[c].tm = o.tm_pm; cand[c].hairpin_tm = o.tm_hairpin; cand[c].homodimer_tm = o.tm_dimer; cand[c].dG = thermo_delta_g(o);
	ok[c] = thermo_expansion_valid(o, a, check_homo) ? 1u : 0u;
}

// first rank key: more records first (n_records - records < 2^31); ord[c] = c
__global__ void k_pc_key_records(const pcr_probe_candidate *__restrict__ cand, uint32_t n, uint32_t n_records, uint32_t *__restrict__ key, uint32_t *__restrict__ ord)
{
	const uint32_t c = blockIdx.x*blockDim.x + threadIdx.x;
	if(c < n){ key[c] = n_records - cand[c].records; ord[c] = c; }
}

// second rank key: the group (PC_DROPPED for a candidate that is not ok), then more sequences first
__global__ void k_pc_key_group(const pcr_probe_candidate *__restrict__ cand, const uint32_t *__restrict__ ok, const uint32_t *__restrict__ ord, uint32_t n,
	uint32_t n_sequences, uint64_t *__restrict__ key)
{
	const uint32_t i = blockIdx.x*blockDim.x + threadIdx.x;
	if(i >= n) return;
	const uint32_t c = ord[i];
	const uint32_t g = (ok && !ok[c]) ? PC_DROPPED : cand[c].group;
	key[i] = ((uint64_t)g << 32) | (uint64_t)(n_sequences - cand[c].sequences);
}

// ranked position i -> i where a group starts, else 0 (an inclusive max-scan then gives every position its group's start)
__global__ void k_pc_group_heads(const uint64_t *__restrict__ key, uint32_t n, uint32_t *__restrict__ head_pos)
{
	const uint32_t i = blockIdx.x*blockDim.x + threadIdx.x;
	if(i < n) head_pos[i] = (i > 0 && (key[i] >> 32) != (key[i - 1] >> 32)) ? i : 0u;
}

// keep[i] = the candidate at ranked position i is ok and among the first per_group of its group (keep[n] = 0 closes the scan)
__global__ void k_pc_cut(const uint64_t *__restrict__ key, const uint32_t *__restrict__ group_start, uint32_t n, uint32_t per_group, uint32_t *__restrict__ keep)
{
	const uint32_t i = blockIdx.x*blockDim.x + threadIdx.x;
	if(i > n) return;
	if(i == n){ keep[i] = 0u; return; }
	keep[i] = ((uint32_t)(key[i] >> 32) != PC_DROPPED && (per_group == 0u || i - group_start[i] < per_group)) ? 1u : 0u;
}

__global__ void k_pc_write(const uint32_t *__restrict__ keep, const uint32_t *__restrict__ keep_scan, const uint32_t *__restrict__ ord,
	const pcr_probe_candidate *__restrict__ cand, uint32_t n, pcr_probe_candidate *__restrict__ out)
{
	const uint32_t i = blockIdx.x*blockDim.x + threadIdx.x;
	if(i < n && keep[i]) out[keep_scan[i]] = cand[ord[i]];
}

inline unsigned pc_bits(uint64_t max_value) { unsigned b = 1; while(b < 64 && (max_value >> b)) ++b; return b; }

// a rocprim device primitive on the handle's stream with its scratch in ppc_tmp: f(scratch, bytes) is called twice
template<class F> int pc_prim(pcr_ctx *ctx, F f)
{
	size_t bytes = 0;
	HIP_TRY(f((void *)nullptr, bytes));
	const int rc = ctx->ppc_tmp.ensure(bytes + 16);
	if(rc != PCR_OK) return rc;
	HIP_TRY(f((void *)ctx->ppc_tmp.p, bytes));
	return PCR_OK;
}
template<class K> int pc_sort(pcr_ctx *ctx, K *k_in, K *k_out, uint32_t *v_in, uint32_t *v_out, uint32_t n, unsigned bits)
{
	return pc_prim(ctx, [&](void *t, size_t &b){ return rocprim::radix_sort_pairs(t, b, k_in, k_out, v_in, v_out, n, 0, bits, ctx->stream); });
}
template<class T> int pc_exclusive_sum(pcr_ctx *ctx, T *in, T *out, size_t n)
{
	return pc_prim(ctx, [&](void *t, size_t &b){ return rocprim::exclusive_scan(t, b, in, out, T(0), n, rocprim::plus<T>(), ctx->stream); });
}

} // namespace

extern "C" {

int64_t pcr_pool_probe_candidates(pcr_ctx *ctx, pcr_set which, const pcr_product *products, const uint32_t *group, uint64_t n,
	uint32_t len_min, uint32_t len_max, uint32_t strands, uint32_t rules, uint32_t max_run, float gc_min, float gc_max,
	uint32_t min_sequences, const pcr_thermo_args *args, int check_homo_dimer, uint32_t per_group,
	pcr_probe_candidate *out, uint64_t cap)
{
	static_assert(sizeof(pcr_probe_candidate) == 64, "record layout");
	const char *const who = "pcr_pool_probe_candidates";
	// ---- the arguments, before the handle
	if(!set_ok(which)){ g_err = std::string(who) + ": unknown sequence set"; return PCR_ERR_ARG; }
	if(which != PCR_SET_TARGET && which != PCR_SET_BACKGROUND){ g_err = std::string(who) + ": PCR_SET_MULTIPLEX is not supported (PCR_SET_TARGET or PCR_SET_BACKGROUND)"; return PCR_ERR_ARG; }
	if((n && !products) || (cap && !out)){ g_err = std::string(who) + ": bad argument"; return PCR_ERR_ARG; }
	if(n >= (1ull << 31)){ g_err = std::string(who) + ": 2^31 or more records"; return PCR_ERR_ARG; }
	if(len_min < 1 || len_min > len_max || len_max > 32){ g_err = std::string(who) + ": lengths outside 1 <= len_min <= len_max <= 32"; return PCR_ERR_ARG; }
	if(strands < 1 || strands > 3){ g_err = std::string(who) + ": strands must be 1, 2 or 3"; return PCR_ERR_ARG; }
	if(rules & ~(PCR_PROBE_NO_5G | PCR_PROBE_C_GE_G)){ g_err = std::string(who) + ": unknown rule bits"; return PCR_ERR_ARG; }
	if(!std::isfinite(gc_min) || !std::isfinite(gc_max) || gc_min > gc_max){ g_err = std::string(who) + ": gc_min and gc_max must be finite with gc_min <= gc_max"; return PCR_ERR_ARG; }
	if(args){
		if(!(args->primer_strand > 0.0f)){ g_err = std::string(who) + ": primer_strand (the probe's concentration) must be positive"; return PCR_ERR_ARG; }
		if(!(args->salt >= 1.0e-6f && args->salt <= 1.0f)){ g_err = std::string(who) + ": salt outside [1e-6, 1] (NucCruc::salt, nuc_cruc.h:780-788)"; return PCR_ERR_ARG; }
	}
	if(!ctx){ g_err = std::string(who) + ": null handle"; return PCR_ERR_ARG; }
	{ const int drc = drain(ctx); if(drc != PCR_OK) return drc; }
	HIP_TRY(hipSetDevice(ctx->device));
	const uint32_t nr = (uint32_t)n;
	if(group){
		for(uint32_t k = 0;k < nr;++k) if(group[k] >= PCR_POOL_MAX_PAIRS && group[k] != PCR_NO_GROUP){
			g_err = std::string(who) + ": record " + std::to_string(k) + ": group " + std::to_string(group[k]) + " is neither below PCR_POOL_MAX_PAIRS nor PCR_NO_GROUP";
			return PCR_ERR_ARG;
		}
	}
	SeqSet &S = ctx->sets[which];
	if(S.n == 0){ g_err = std::string(who) + ": the set is not loaded (call pcr_load_sequences first)"; return PCR_ERR_STATE; }
	if(n == 0) return 0;
	// ---- every participating record's insert, against the set's lengths: no kernel sees one that fails; then the windows
	std::vector<uint4> iv(nr);
	for(uint32_t k = 0;k < nr;++k){
		const uint32_t g = group ? group[k] : 0u;
		if(g == PCR_NO_GROUP){ iv[k] = make_uint4(0u, 0u, 0u, g); continue; }       // (no start position: no lane ever reads it)
		const int irc = product_interval(who, S, products[k], k, PCR_REGION_INSERT, iv[k]);
		if(irc != PCR_OK) return irc;
		iv[k].w = g;
	}
	const uint32_t n_strands = (strands == 3u) ? 2u : 1u;
	std::vector<uint32_t> pos_off((size_t)nr + 1);
	uint64_t windows = 0, n_pos64 = 0;
	for(uint32_t k = 0;k < nr;++k){
		pos_off[k] = (uint32_t)n_pos64;
		const uint64_t I = (iv[k].w == PCR_NO_GROUP) ? 0 : iv[k].z;
		if(I < len_min) continue;
		const uint64_t top = std::min<uint64_t>(len_max, I), count = top - len_min + 1;   // L = len_min .. top: I - L + 1 windows each
		windows += n_strands*(count*(I + 1) - (top*(top + 1) - (uint64_t)len_min*(len_min - 1))/2);
		n_pos64 += I - len_min + 1;
		if(windows >= PC_MAX_WINDOWS){ g_err = std::string(who) + ": 2^28 or more windows to enumerate (by record " + std::to_string(k) + ")"; return PCR_ERR_CAPACITY; }
	}
	pos_off[nr] = (uint32_t)n_pos64;
	if(n_pos64 == 0) return 0;
	const uint32_t n_pos = (uint32_t)n_pos64, n_chunks = (n_pos + PC_THREADS - 1)/PC_THREADS;
	// ---- 1. count, scan, emit
	int rc;
	if((rc = ctx->ppc_iv.ensure(nr)) != PCR_OK) return rc;
	if((rc = ctx->ppc_pos.ensure((size_t)nr + 1 + 2*((size_t)n_chunks + 1) + 1)) != PCR_OK) return rc;
	uint32_t *d_pos_off = ctx->ppc_pos.p, *chunk_cnt = d_pos_off + nr + 1, *chunk_off = chunk_cnt + n_chunks + 1, *flag = chunk_off + n_chunks + 1;
	PcFence fence{ctx->stream};                                                   // iv and pos_off are pageable: no return leaves a copy of them pending
	HIP_TRY(hipMemcpyAsync(ctx->ppc_iv.p, iv.data(), (size_t)nr*sizeof(uint4), hipMemcpyHostToDevice, ctx->stream));
	HIP_TRY(hipMemcpyAsync(d_pos_off, pos_off.data(), ((size_t)nr + 1)*sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
	HIP_TRY(hipMemsetAsync(chunk_cnt + n_chunks, 0, sizeof(uint32_t), ctx->stream));
	HIP_TRY(hipMemsetAsync(flag, 0, sizeof(uint32_t), ctx->stream));
	const ProbeRules R = { len_min, len_max, strands, rules, max_run, gc_min, gc_max };
	const unsigned grid_e = std::max(1u, std::min<unsigned>(n_chunks, ctx->n_cu*PC_BLOCKS_PER_CU));
	const uint4 *d_planes = (const uint4 *)S.planes.p;
	const uint64_t *d_blk = (const uint64_t *)S.d_blk_off.p;
	hipLaunchKernelGGL(k_pc_enumerate<false>, dim3(grid_e), dim3(PC_THREADS), 0, ctx->stream, d_planes, d_blk, (const uint4 *)ctx->ppc_iv.p, (const uint32_t *)d_pos_off,
		nr, n_pos, n_chunks, R, chunk_cnt, (const uint32_t *)nullptr, 0u, (uint64_t *)nullptr, (uint32_t *)nullptr, (uint32_t *)nullptr, (uint32_t *)nullptr);
	HIP_TRY(hipGetLastError());
	if((rc = pc_exclusive_sum(ctx, chunk_cnt, chunk_off, (size_t)n_chunks + 1)) != PCR_OK) return rc;
	uint32_t n_occ = 0;
	HIP_TRY(hipMemcpyAsync(&n_occ, chunk_off + n_chunks, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
	HIP_TRY(hipStreamSynchronize(ctx->stream));
	fence.armed = false;                                                          // (iv and pos_off are read by now)
	if(n_occ == 0) return 0;
	const size_t O = n_occ, O1 = O + 1;
	if((rc = ctx->ppc_u32.ensure(3*O + 4*O1)) != PCR_OK) return rc;
	if((rc = ctx->ppc_u64.ensure(O + 2*O1)) != PCR_OK) return rc;
	uint32_t *o_rec = ctx->ppc_u32.p, *o_pos = o_rec + O, *o_gls = o_pos + O, *a0 = o_gls + O, *a1 = a0 + O1, *v0 = a1 + O1, *v1 = v0 + O1;
	uint64_t *o_spell = ctx->ppc_u64.p, *k0 = o_spell + O, *k1 = k0 + O1;
	hipLaunchKernelGGL(k_pc_enumerate<true>, dim3(grid_e), dim3(PC_THREADS), 0, ctx->stream, d_planes, d_blk, (const uint4 *)ctx->ppc_iv.p, (const uint32_t *)d_pos_off,
		nr, n_pos, n_chunks, R, (uint32_t *)nullptr, (const uint32_t *)chunk_off, n_occ, o_spell, o_rec, o_pos, o_gls);
	HIP_TRY(hipGetLastError());
	// ---- 2. the index sorted by (group, L, spelling, sequence, record, start, strand); runs, and the changes inside them
	const unsigned grid_o = (unsigned)((O1 + 255)/256);
	hipLaunchKernelGGL(k_pc_key_seq, dim3(grid_o), dim3(256), 0, ctx->stream, (const uint4 *)ctx->ppc_iv.p, (const uint32_t *)o_rec, n_occ, a0, v0);
	HIP_TRY(hipGetLastError());
	if((rc = pc_sort(ctx, a0, a1, v0, v1, n_occ, pc_bits(S.n - 1))) != PCR_OK) return rc;
	hipLaunchKernelGGL(k_pc_key_spell, dim3(grid_o), dim3(256), 0, ctx->stream, (const uint64_t *)o_spell, (const uint32_t *)v1, n_occ, k0);
	HIP_TRY(hipGetLastError());
	if((rc = pc_sort(ctx, k0, k1, v1, v0, n_occ, 2*len_max)) != PCR_OK) return rc;
	hipLaunchKernelGGL(k_pc_key_gl, dim3(grid_o), dim3(256), 0, ctx->stream, (const uint32_t *)o_gls, (const uint32_t *)v0, n_occ, a0);
	HIP_TRY(hipGetLastError());
	if((rc = pc_sort(ctx, a0, a1, v0, v1, n_occ, 15)) != PCR_OK) return rc;       // 10 bits of group, 5 of L - 1
	const uint32_t *ord = v1;
	hipLaunchKernelGGL(k_pc_flags, dim3(grid_o), dim3(256), 0, ctx->stream, (const uint4 *)ctx->ppc_iv.p, (const uint64_t *)o_spell, (const uint32_t *)o_rec,
		(const uint32_t *)o_gls, ord, n_occ, a0, k0);
	HIP_TRY(hipGetLastError());
	if((rc = pc_exclusive_sum(ctx, a0, a1, O1)) != PCR_OK) return rc;             // a1: the run of every position, a1[O] their number
	if((rc = pc_exclusive_sum(ctx, k0, k1, O1)) != PCR_OK) return rc;             // k1: sequence | record changes before every position
	uint32_t *run_start = v0;
	hipLaunchKernelGGL(k_pc_run_start, dim3(grid_o), dim3(256), 0, ctx->stream, (const uint32_t *)a0, (const uint32_t *)a1, n_occ, run_start);
	HIP_TRY(hipGetLastError());
	uint32_t n_runs = 0;
	HIP_TRY(hipMemcpyAsync(&n_runs, a1 + O, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
	HIP_TRY(hipStreamSynchronize(ctx->stream));
	// ---- 3. the runs that enough sequences hold; their records; the engine's verdict
	const unsigned grid_r = (n_runs + 1 + 255)/256;
	hipLaunchKernelGGL(k_pc_run_keep, dim3(grid_r), dim3(256), 0, ctx->stream, (const uint32_t *)run_start, (const uint64_t *)k1, n_runs, min_sequences, a0);
	HIP_TRY(hipGetLastError());
	if((rc = pc_exclusive_sum(ctx, a0, a1, (size_t)n_runs + 1)) != PCR_OK) return rc;
	uint32_t n_cand = 0;
	HIP_TRY(hipMemcpyAsync(&n_cand, a1 + n_runs, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
	HIP_TRY(hipStreamSynchronize(ctx->stream));
	if(n_cand == 0) return 0;
	if((rc = ctx->ppc_rec.ensure(2*(size_t)n_cand)) != PCR_OK) return rc;
	pcr_probe_candidate *cand = ctx->ppc_rec.p, *kept = cand + n_cand;
	hipLaunchKernelGGL(k_pc_cand, dim3(grid_r), dim3(256), 0, ctx->stream, (const uint32_t *)a0, (const uint32_t *)a1, (const uint32_t *)run_start,
		(const uint64_t *)k1, ord, (const uint64_t *)o_spell, (const uint32_t *)o_rec, (const uint32_t *)o_pos, (const uint32_t *)o_gls, n_runs, cand, k0);
	HIP_TRY(hipGetLastError());
	const unsigned grid_c = (n_cand + 1 + 255)/256;
	uint32_t *ok = nullptr;
	if(args){
		const size_t n_mirror = check_homo_dimer ? n_cand : 0;
		if((rc = ctx->th_jobs.ensure(n_cand)) != PCR_OK) return rc;
		if((rc = ctx->th_out.ensure(n_cand + n_mirror + 1)) != PCR_OK) return rc;
		if((rc = ensure_dg_table(ctx, args->salt)) != PCR_OK) return rc;
		hipLaunchKernelGGL(k_pc_jobs, dim3(grid_c), dim3(256), 0, ctx->stream, (const pcr_probe_candidate *)cand, (const uint64_t *)k0, n_cand, check_homo_dimer,
			logf((float)(args->primer_strand/1.0)), ctx->th_jobs.p);
		HIP_TRY(hipGetLastError());
		const thermo::ThermoValid plain = { nullptr, nullptr, 0.0f, 0.0f, 0.0f };
		if((rc = launch_thermo(ctx, ctx->th_jobs.p, n_cand, n_mirror, logf(args->salt), plain)) != PCR_OK) return rc;
		ok = v1;                                                                   // (the sorted index is spent)
		hipLaunchKernelGGL(k_pc_verdict, dim3(grid_c), dim3(256), 0, ctx->stream, (const thermo::JobOut *)ctx->th_out.p, n_cand, check_homo_dimer, *args, cand, ok, flag);
		HIP_TRY(hipGetLastError());
	}
	// ---- 4. rank inside each group, cut, gather.  Everything but cand[] and ok[] (= v1) is spent; n_cand + 1 <= O + 1 entries each.
	uint32_t *idx = v0, *idx2 = o_rec;                                            // (o_rec has O >= n_cand entries)
	hipLaunchKernelGGL(k_pc_key_records, dim3(grid_c), dim3(256), 0, ctx->stream, (const pcr_probe_candidate *)cand, n_cand, nr, a0, idx);
	HIP_TRY(hipGetLastError());
	if((rc = pc_sort(ctx, a0, a1, idx, idx2, n_cand, pc_bits(nr))) != PCR_OK) return rc;
	hipLaunchKernelGGL(k_pc_key_group, dim3(grid_c), dim3(256), 0, ctx->stream, (const pcr_probe_candidate *)cand, (const uint32_t *)ok, (const uint32_t *)idx2, n_cand,
		S.n, k1);
	HIP_TRY(hipGetLastError());
	if((rc = pc_sort(ctx, k1, k0, idx2, idx, n_cand, 32 + 11)) != PCR_OK) return rc;   // k0: the ranked keys, idx: the ranked candidates
	hipLaunchKernelGGL(k_pc_group_heads, dim3(grid_c), dim3(256), 0, ctx->stream, (const uint64_t *)k0, n_cand, a0);
	HIP_TRY(hipGetLastError());
	if((rc = pc_prim(ctx, [&](void *t, size_t &b){ return rocprim::inclusive_scan(t, b, a0, a1, (size_t)n_cand, rocprim::maximum<uint32_t>(), ctx->stream); })) != PCR_OK) return rc;
	uint32_t *keep = a0, *keep_scan = v1;                                         // (the group heads are scanned, ok[] is in the keys)
	hipLaunchKernelGGL(k_pc_cut, dim3(grid_c), dim3(256), 0, ctx->stream, (const uint64_t *)k0, (const uint32_t *)a1, n_cand, per_group, keep);
	HIP_TRY(hipGetLastError());
	if((rc = pc_exclusive_sum(ctx, keep, keep_scan, (size_t)n_cand + 1)) != PCR_OK) return rc;
	hipLaunchKernelGGL(k_pc_write, dim3(grid_c), dim3(256), 0, ctx->stream, (const uint32_t *)keep, (const uint32_t *)keep_scan, (const uint32_t *)idx,
		(const pcr_probe_candidate *)cand, n_cand, kept);
	HIP_TRY(hipGetLastError());
	uint32_t total = 0, bad = 0;
	HIP_TRY(hipMemcpyAsync(&total, keep_scan + n_cand, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
	HIP_TRY(hipMemcpyAsync(&bad, flag, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
	HIP_TRY(hipStreamSynchronize(ctx->stream));
	if(bad & 1u){ g_err = std::string(who) + ": internal trace-back error"; return PCR_ERR_RANGE; }
	if(total && total <= cap){
		HIP_TRY(hipMemcpyAsync(out, kept, (size_t)total*sizeof(pcr_probe_candidate), hipMemcpyDeviceToHost, ctx->stream));
		HIP_TRY(hipStreamSynchronize(ctx->stream));
	}
	return (int64_t)total;
}

} // extern "C"
