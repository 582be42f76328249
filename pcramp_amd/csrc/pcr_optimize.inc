// The local search of the reference's optimiser behind the C-ABI, batched over trial assays (included by
// pcr_entry_sw_thermo.inc).
//
// Reference: optimize() and optimization_move() (optimize.cpp:14-207, 303-352), the six moves of optimize_pcr.cpp
// (:8-989), Score (pcramp.h:158-208), the per-trial parallel loop of main.cpp:697-887 that runs optimize() for every
// one of the num_trial assays of a design iteration.
//
// All assays advance in lockstep, one optimiser iteration at a time.  Per iteration and for ALL assays still searching:
//   * the trial words of every move of both oligos are listed on the host (pcrhost::move_trials: the reference's order
//     and gates);
//   * ONE thermodynamics launch decides PCR::is_valid for every trial word of every assay (run_thermo_jobs);
//   * ONE move-coverage pass per sequence set (k_match over the base oligos of all assays, k_pair_moves_batch,
//     k_cov_from_bits) gives compute_coverage for the unmodified assays and every valid trial; with opt.use_multiplex one
//     k_key_coverage_batch launch gives the multiplex background term;
//   * the moves are decided on the host in the reference's order with its Score arithmetic (float, compared through
//     accuracy = target - background, then oligo_overlap).
// Coverage does not depend on the running score threshold, so evaluating all trials before deciding equals the reference's
// one-trial-at-a-time loop.

namespace {

struct MoveJob { uint32_t v_begin, v_end; };   // variants[v_begin .. v_end) belong to oligo 2*assay + side
static_assert(sizeof(MoveJob) == sizeof(uint2), "job records travel in a uint2 buffer");

// k_match (pcr_screen.inc) with the layout the batched sweep wants: the mask words TRANSPOSED (word w of all slots
// contiguous: a sweep over the partners of a site reads one word per partner, 4 bytes apart instead of 4 * mask_words) and
// a compact loc | strand << 31 per slot (instead of a field of the 48-byte entry).  One wave per touched sequence, a lane =
// (entry parity, oligo % 32).
__global__ __launch_bounds__(64*MATCH_WAVES) void k_match_t(const DevEntry *__restrict__ db, uint32_t n_touched, uint32_t cap,
	const uint32_t *__restrict__ touched, const uint32_t *__restrict__ seg_hi, const OligoDev *__restrict__ oligos, uint32_t n_oligo,
	uint32_t mask_words, uint64_t n_slots, uint32_t *__restrict__ mask_t, uint32_t *__restrict__ loc_strand, uint32_t *__restrict__ status)
{
	if(blockIdx.x == 0 && threadIdx.x == 0 && status) status[0] = 0;
	const uint32_t lane = threadIdx.x & 63u, sub = lane >> 5, ol = lane & 31u;
	for(uint32_t t_idx = blockIdx.x*MATCH_WAVES + (threadIdx.x >> 6);t_idx < n_touched;t_idx += gridDim.x*MATCH_WAVES){
		const uint32_t seq = touched[t_idx];
		const uint32_t lo = seq*cap, n_e = seg_hi[seq] - lo;
		for(uint32_t e0 = 0;e0 < n_e;e0 += 2){
			const bool have = e0 + sub < n_e;
			const uint32_t i = lo + e0 + sub;
			Planes w; w.a = w.c = w.g = w.t = 0;
			if(have){
				w = db[i].w;
				if(ol == 0) loc_strand[i] = ((uint32_t)(db[i].loc + LOC_BIAS) & 0x7FFFFFFFu) | ((db[i].strand == 2u) ? 0x80000000u : 0u);
			}
			for(uint32_t mw = 0;mw < mask_words;++mw){
				const uint32_t o = mw*32 + ol;
				bool ok = false;
				if(have && o < n_oligo){
					const Planes m = oligos[o].m;
					ok = (uint32_t)__popc((w.a & m.a) | (w.c & m.c) | (w.g & m.g) | (w.t & m.t)) >= oligos[o].floor2;
				}
				const uint64_t bal = __ballot(ok);
				if(have && ol == 0) mask_t[(size_t)mw*n_slots + i] = sub ? (uint32_t)(bal >> 32) : (uint32_t)bal;
			}
		}
	}
}

// the same for at most 32 oligos (a single assay, a few): a thread per DB slot instead of a wave per sequence -- k_match's lane
// layout would walk a 2 048-slot bucket in 1 024 steps with 60 lanes idle (k_match_few, pcr_screen.inc)
__global__ void k_match_few_t(const DevEntry *__restrict__ db, uint32_t n, uint32_t cap, const uint32_t *__restrict__ touched,
	const uint32_t *__restrict__ seg_hi, const OligoDev *__restrict__ oligos, uint32_t n_oligo, uint32_t *__restrict__ mask_t,
	uint32_t *__restrict__ loc_strand, uint32_t *__restrict__ status)
{
	__shared__ OligoDev sh[32];
	if(blockIdx.x == 0 && threadIdx.x == 0 && status) status[0] = 0;
	for(uint32_t i = threadIdx.x;i < n_oligo*(uint32_t)(sizeof(OligoDev)/4);i += blockDim.x) ((uint32_t *)sh)[i] = ((const uint32_t *)oligos)[i];
	__syncthreads();
	uint32_t e;
	if(!db_slot(blockIdx.x*blockDim.x + threadIdx.x, n, cap, touched, seg_hi, e)) return;
	const DevEntry d = db[e];
	uint32_t m = 0;
	for(uint32_t o = 0;o < n_oligo;++o){
		const Planes q = sh[o].m;
		if((uint32_t)__popc((d.w.a & q.a) | (d.w.c & q.c) | (d.w.g & q.g) | (d.w.t & q.t)) >= sh[o].floor2) m |= 1u << o;
	}
	mask_t[e] = m;
	loc_strand[e] = ((uint32_t)(d.loc + LOC_BIAS) & 0x7FFFFFFFu) | ((d.strand == 2u) ? 0x80000000u : 0u);
}

// (entry, base oligo) pairs with an admissible amplicon: their trial words are evaluated by k_pair_moves_tasks
struct MoveTask { uint32_t entry; uint32_t oligo_orient; float best; };      // DB slot | base oligo (bit 31: orientation 1 = {R plus, F minus}) | largest identity of the OTHER oligo over the admissible partners
constexpr uint32_t PM_THREADS = 128, PM_WG_TASKS = 768;

// k_pair_moves (pcr_screen.inc) for many assays at once: a thread owns one DB entry; every base oligo that matches it
// (bit o = 2*assay + side of its mask words) makes the entry a site of that oligo, handled exactly as k_pair_moves does
// for its one assay: the largest identity of the OTHER oligo over the admissible partners, then one identity per trial
// word of (assay, side).
__global__ void k_pair_moves_batch(const DevEntry *__restrict__ db, uint32_t n, uint32_t cap, const uint32_t *__restrict__ touched,
	const uint32_t *__restrict__ seg_hi, const uint32_t *__restrict__ mask_t, const uint32_t *__restrict__ loc_strand, uint32_t mask_words, uint64_t n_slots,
	const OligoDev *__restrict__ base, uint32_t n_oligo, const MoveJob *__restrict__ jobs, const OligoDev *__restrict__ variants,
	const uint4 *__restrict__ planes, const uint64_t *__restrict__ blk_off, const uint64_t *__restrict__ len,
	const uint8_t *__restrict__ active, const uint8_t *__restrict__ has_eos, int32_t amp_min, int32_t amp_max, float ident_thr, int use_taq,
	uint64_t *__restrict__ bits_fr, uint64_t *__restrict__ bits_rf, uint64_t bit_words, uint32_t *__restrict__ status,
	MoveTask *__restrict__ tasks, uint32_t *__restrict__ task_count, uint32_t task_cap, uint32_t wg_cap /* <= PM_WG_TASKS; smaller only under the test hook */)
{
	// The trial words of an (entry, oligo) pair with an admissible amplicon are NOT walked here (one lane would walk ~100 of them
	// while the other 63 of its wave wait: that loop was most of the 7e8 VALU instructions of a launch on a dense background
	// DB): the pair becomes a task for k_pair_moves_tasks.  Tasks are gathered per workgroup in LDS and appended to the global list
	// with one atomic per workgroup (one per task, all on one counter, cost as much as the loop had).
	__shared__ MoveTask wg_tasks[PM_WG_TASKS];
	__shared__ uint32_t wg_n, wg_base;
	if(threadIdx.x == 0) wg_n = 0;
	__syncthreads();
	const uint32_t t = blockIdx.x*blockDim.x + threadIdx.x;
	uint32_t e = 0;
	const bool mine = db_slot(t, n, cap, touched, seg_hi, e);
	auto work = [&](){
	const DevEntry ee = db[e];
	if(!active[ee.seq]) return;                                                  // optimize.cpp:281
	const uint32_t lo = ee.seq*cap, hi = seg_hi[ee.seq];
	const int32_t L = (int32_t)len[ee.seq];
	const uint64_t blk_base = blk_off[ee.seq];
	const bool eos = has_eos[ee.seq] != 0;
	const bool plus_role = (ee.strand == 1);
	const uint64_t bit = 1ull << (ee.seq & 63);
	for(uint32_t w = 0;w < mask_words;++w){
		const uint32_t *mrow = mask_t + (size_t)w*n_slots;                          // this word of every slot
		uint32_t m = mrow[e];
		while(m){
			const uint32_t b = (uint32_t)__ffs(m) - 1u; m &= m - 1;
			const uint32_t o = w*32 + b;
			if(o >= n_oligo) break;
			const MoveJob job = jobs[o];
			if(job.v_begin == job.v_end) continue;
			const int side = (int)(o & 1u);
			const OligoDev F = base[o & ~1u], R = base[o | 1u];
			const int orient = plus_role ? side : 1 - side;                          // 0 = {F plus, R minus}, 1 = {R plus, F minus}
			const OligoDev &P = (orient == 0) ? F : R;
			const OligoDev &M = (orient == 0) ? R : F;
			const OligoDev &other = (side == 0) ? R : F;
			const uint32_t other_bit = b ^ 1u;
			float best = -1.0f;
			for(int64_t q = plus_role ? (int64_t)e + 1 : (int64_t)e - 1;plus_role ? (q < (int64_t)hi) : (q >= (int64_t)lo);q += plus_role ? 1 : -1){
				const uint32_t ls = loc_strand[q];
				const int32_t ploc = (int32_t)(ls & 0x7FFFFFFFu) - LOC_BIAS;
				const int32_t iloc = plus_role ? ee.loc : ploc, jloc = plus_role ? ploc : ee.loc;
				if(jloc - iloc > amp_max + 128) break;                               // beyond any admissible amplicon (as k_pair)
				if(!((mrow[q] >> other_bit) & 1u)) continue;
				if((ls >> 31) != (plus_role ? 1u : 0u)) continue;                    // the partner sits on the other strand
				if(iloc + P.stop >= jloc - M.stop) continue;                         // pcr_assay.cpp:367-370
				int32_t amp_start = iloc + P.start;
				const int32_t amp_stop = min(jloc - M.start, L - 1);
				int32_t amp_len = amp_stop - amp_start + 1;
				if(amp_len < amp_min || amp_len > amp_max) continue;
				if(amp_start < 0){ amp_len += amp_start; amp_start = 0; }
				if(amp_len < 0 || amp_start + amp_len > L){ atomicOr(status, 1u); continue; }   // sequence.cpp:306 throw
				if(eos && has_split(planes, blk_base, amp_start, amp_len)) continue;
				best = fmaxf(best, identity(other, db[q].w, use_taq));
			}
			if(best < 0.0f) continue;                                                // no admissible amplicon through this entry
			const uint32_t slot = atomicAdd(&wg_n, 1u);
			if(slot < wg_cap){ MoveTask tk; tk.entry = e; tk.oligo_orient = o | ((uint32_t)orient << 31); tk.best = best; wg_tasks[slot] = tk; continue; }
			uint64_t *dst = (orient == 0) ? bits_fr : bits_rf;                        // the workgroup's list is full: in place
			for(uint32_t v = job.v_begin;v < job.v_end;++v){
				const float var = identity(variants[v], ee.w, use_taq);
				const float f = (side == 0) ? var : best, r = (side == 0) ? best : var;
				if(sqrtf(__fmul_rn(f, r)) >= ident_thr)                         // pcr_assay.cpp:285-287
					atomicOr((unsigned long long *)&dst[(size_t)v*bit_words + (ee.seq >> 6)], bit);
			}
		}
	}
	};
	if(mine) work();
	__syncthreads();
	const uint32_t n_mine = min(wg_n, wg_cap);
	if(threadIdx.x == 0 && n_mine) wg_base = atomicAdd(&task_count[0], n_mine);
	__syncthreads();
	for(uint32_t i = threadIdx.x;i < n_mine;i += blockDim.x){
		const MoveTask tk = wg_tasks[i];
		const uint32_t slot = wg_base + i;
		if(slot < task_cap){ tasks[slot] = tk; continue; }
		// the global list is full (it holds 4 tasks per DB slot): this task in place
		const uint32_t o = tk.oligo_orient & 0x7FFFFFFFu;
		const int side = (int)(o & 1u);
		const MoveJob job = jobs[o];
		const DevEntry ee = db[tk.entry];
		uint64_t *dst = (tk.oligo_orient >> 31) ? bits_rf : bits_fr;
		for(uint32_t v = job.v_begin;v < job.v_end;++v){
			const float var = identity(variants[v], ee.w, use_taq);
			const float f = (side == 0) ? var : tk.best, r = (side == 0) ? tk.best : var;
			if(sqrtf(__fmul_rn(f, r)) >= ident_thr) atomicOr((unsigned long long *)&dst[(size_t)v*bit_words + (ee.seq >> 6)], 1ull << (ee.seq & 63));
		}
	}
}

// The same with the partner walk out of LDS (the form pcr_optimize_batch launches).  k_pair_moves_batch gives every DB slot a
// thread that walks its partners through global memory -- two dependent loads per partner, ~100 partners per (entry, oligo) on a
// dense background DB (470 entries per sequence, a 2 000-base amplicon window): 2.4 ms per launch, the largest single item of
// pcr_optimize_batch (r03 profile).  Here a GROUP of threads owns a sequence -- a workgroup when the buckets are large (WG_SEQ), a
// wave otherwise -- and first brings the sequence's (position | strand) words into LDS, then, one mask word (32 base oligos = 16
// assays) at a time, that word of every entry; a thread then handles its entries as before, but every partner it looks at costs
// two LDS reads.  Entries, geometry, identity and the task hand-over are k_pair_moves_batch's.
template<bool WG_SEQ>
__global__ __launch_bounds__(256) void k_pair_moves_lds(const DevEntry *__restrict__ db, uint32_t n_touched, uint32_t cap, const uint32_t *__restrict__ touched,
	const uint32_t *__restrict__ seg_hi, const uint32_t *__restrict__ mask_t, const uint32_t *__restrict__ loc_strand, uint32_t mask_words, uint64_t n_slots,
	const OligoDev *__restrict__ base, uint32_t n_oligo, const MoveJob *__restrict__ jobs, const OligoDev *__restrict__ variants,
	const uint4 *__restrict__ planes, const uint64_t *__restrict__ blk_off, const uint64_t *__restrict__ len,
	const uint8_t *__restrict__ active, const uint8_t *__restrict__ has_eos, int32_t amp_min, int32_t amp_max, float ident_thr, int use_taq,
	uint64_t *__restrict__ bits_fr, uint64_t *__restrict__ bits_rf, uint64_t bit_words, uint32_t *__restrict__ status,
	MoveTask *__restrict__ tasks, uint32_t *__restrict__ task_count, uint32_t task_cap, uint32_t wg_cap)
{
	extern __shared__ uint32_t pml_lds[];                      // per group: ls[stride] | mw[stride]   (stride = cap for a workgroup, 64 for a wave)
	__shared__ MoveTask wg_tasks[PM_WG_TASKS];
	__shared__ uint32_t wg_n, wg_base;
	// the 32 base oligos of the current mask word as the walk needs them: Word::start() | stop() << 8 | (has trial words) << 16.  (Read
	// from the oligo and job tables per (entry, oligo) these were five global loads in front of every walk: 2 000 memory
	// instructions per wave and launch, 69 % of the wave cycles waiting -- the r03 profile of this kernel.)
	__shared__ uint32_t s_geo[WG_SEQ ? 32 : 1];
	__shared__ OligoDev s_ol[WG_SEQ ? 32 : 1];                                // ... and whole, for the identity of a partner (the compiler hoists the loads of `other` in front of the walk)
	if(threadIdx.x == 0) wg_n = 0;
	__syncthreads();
	const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
	uint32_t *const geo = s_geo;                                                 // (WG_SEQ only)
	OligoDev *const ol = s_ol;
	static_assert(sizeof(OligoDev) == 40, "copied as 10 words");
	const uint32_t group = WG_SEQ ? blockIdx.x : blockIdx.x*4u + wave;
	const uint32_t gt = WG_SEQ ? threadIdx.x : lane, gsize = WG_SEQ ? 256u : 64u, stride = WG_SEQ ? cap : 64u;
	uint32_t *const ls = pml_lds + (WG_SEQ ? 0u : wave*2u*stride), *const mw = ls + stride;
	auto group_sync = [&](){ if constexpr (WG_SEQ) __syncthreads(); else wave_sync(); };
	uint32_t seq = 0, lo = 0, n = 0;
	if(group < n_touched){
		seq = touched[group];
		lo = seq*cap;
		n = active[seq] ? (seg_hi[seq] - lo) : 0u;                                  // optimize.cpp:281
	}
	const int32_t L = (int32_t)len[seq];
	const uint64_t blk_base = blk_off[seq];
	const bool eos = has_eos[seq] != 0;
	const uint64_t bit = 1ull << (seq & 63);
	// WG_SEQ only: the mask word TRANSPOSED -- for each of its 32 oligo bits the set of entries that carry it, as a bitset over the
	// sequence's entries (tb[bit][entry / 32]), ANDed at use with the entries of the partner's strand (sb[0]: plus, sb[1]: minus).  On a
	// dense background DB an (entry, oligo) has ~100 entries inside its amplicon window and one or two of them match the other oligo:
	// walking the set bits instead of the window cut the launch from 2.4 to x ms.
	const uint32_t tw = (stride + 31u)/32u;                                         // words per bitset
	uint32_t *const tb = mw + stride, *const sb = tb + 32u*tw;
	// The workgroup's task list goes to the global list with one atomic.  A workgroup that owns a sequence (WG_SEQ) does this after
	// every mask word: a dense background sequence makes ~1 200 tasks per pass (2.5e6 per launch at 256 assays on 2 000 backgrounds,
	// r03 count) and every task beyond the list's 768 slots took the in-place branch -- one lane looping over ~70 trial words
	// through global memory: 1.7 of the launch's 1.85 ms.  Per mask word a sequence makes ~80.
	auto flush_tasks = [&](){
		__syncthreads();
		const uint32_t n_mine = min(wg_n, wg_cap);
		if(threadIdx.x == 0 && n_mine) wg_base = atomicAdd(&task_count[0], n_mine);
		__syncthreads();
		for(uint32_t i = threadIdx.x;i < n_mine;i += blockDim.x){
			const MoveTask tk = wg_tasks[i];
			const uint32_t slot = wg_base + i;
			if(slot < task_cap){ tasks[slot] = tk; continue; }
			// the global list is full (it holds 4 tasks per DB slot): this task in place
			const uint32_t o = tk.oligo_orient & 0x7FFFFFFFu;
			const int side = (int)(o & 1u);
			const MoveJob job = jobs[o];
			const DevEntry ee = db[tk.entry];
			uint64_t *dst = (tk.oligo_orient >> 31) ? bits_rf : bits_fr;
			for(uint32_t v = job.v_begin;v < job.v_end;++v){
				const float var = identity(variants[v], ee.w, use_taq);
				const float f = (side == 0) ? var : tk.best, r = (side == 0) ? tk.best : var;
				if(sqrtf(__fmul_rn(f, r)) >= ident_thr) atomicOr((unsigned long long *)&dst[(size_t)v*bit_words + (ee.seq >> 6)], 1ull << (ee.seq & 63));
			}
		}
		__syncthreads();
		if(threadIdx.x == 0) wg_n = 0;
		__syncthreads();
	};
	for(uint32_t k = gt;k < n;k += gsize) ls[k] = loc_strand[lo + k];
	if constexpr (WG_SEQ){
		for(uint32_t k = gt;k < 2u*tw;k += gsize) sb[k] = 0u;
		group_sync();
		for(uint32_t k = gt;k < n;k += gsize) atomicOr(&sb[(ls[k] >> 31)*tw + (k >> 5)], 1u << (k & 31u));
	}
	for(uint32_t w = 0;w < mask_words;++w){
		group_sync();                                                               // the previous word's walks are over (first round: ls is complete)
		for(uint32_t k = gt;k < n;k += gsize) mw[k] = mask_t[(size_t)w*n_slots + lo + k];
		if constexpr (WG_SEQ){                                                     // (a wave-sized bucket rarely holds a match at all: it reads these per match instead)
			if(gt < 32u){
				const uint32_t o = w*32u + gt;
				uint32_t g = 0;
				if(o < n_oligo){
					const MoveJob job = jobs[o];
					g = ((uint32_t)base[o].start & 0xFFu) | (((uint32_t)base[o].stop & 0xFFu) << 8) | ((job.v_begin != job.v_end) ? (1u << 16) : 0u);
				}
				geo[gt] = g;
			}
			for(uint32_t k = gt;k < 320u;k += gsize){
				const uint32_t o = w*32u + k/10u;
				((uint32_t *)ol)[k] = (o < n_oligo) ? ((const uint32_t *)base)[(size_t)w*320u + k] : 0u;
			}
		}
		if constexpr (WG_SEQ){
			for(uint32_t k = gt;k < 32u*tw;k += gsize) tb[k] = 0u;
			group_sync();
			for(uint32_t k = gt;k < n;k += gsize){
				for(uint32_t m = mw[k];m;m &= m - 1) atomicOr(&tb[((uint32_t)__ffs(m) - 1u)*tw + (k >> 5)], 1u << (k & 31u));
			}
		}
		group_sync();
		for(uint32_t k = gt;k < n;k += gsize){
			uint32_t m = mw[k];
			if(!m) continue;
			const uint32_t els = ls[k];
			const bool plus_role = (els >> 31) == 0;
			const int32_t eloc = (int32_t)(els & 0x7FFFFFFFu) - LOC_BIAS;
			const uint32_t e = lo + k;
			while(m){
				const uint32_t b = (uint32_t)__ffs(m) - 1u; m &= m - 1;
				const uint32_t o = w*32 + b;
				if(o >= n_oligo) break;
				const int side = (int)(o & 1u);
				const int orient = plus_role ? side : 1 - side;                          // 0 = {F plus, R minus}, 1 = {R plus, F minus}
				const uint32_t op = (orient == 0) ? (o & ~1u) : (o | 1u), om = (orient == 0) ? (o | 1u) : (o & ~1u);
				int32_t p_start, p_stop, m_start, m_stop;
				if constexpr (WG_SEQ){
					if(!(geo[b] >> 16)) continue;                                        // no trial words for this oligo
					const uint32_t gp = geo[op & 31u], gm = geo[om & 31u];
					p_start = (int32_t)(int8_t)(gp & 0xFFu); p_stop = (int32_t)(int8_t)((gp >> 8) & 0xFFu);
					m_start = (int32_t)(int8_t)(gm & 0xFFu); m_stop = (int32_t)(int8_t)((gm >> 8) & 0xFFu);
				}
				else{
					const MoveJob job = jobs[o];
					if(job.v_begin == job.v_end) continue;
					p_start = base[op].start; p_stop = base[op].stop; m_start = base[om].start; m_stop = base[om].stop;
				}
				const OligoDev &other = WG_SEQ ? ol[b ^ 1u] : base[o ^ 1u];
				const uint32_t other_bit = b ^ 1u;
				float best = -1.0f;
				// one partner q (index in the sequence) that carries the other oligo's bit and sits on the other strand; false: beyond the window
				auto partner = [&](int32_t q) -> bool {
					const uint32_t qls = ls[q];
					const int32_t ploc = (int32_t)(qls & 0x7FFFFFFFu) - LOC_BIAS;
					const int32_t iloc = plus_role ? eloc : ploc, jloc = plus_role ? ploc : eloc;
					if(jloc - iloc > amp_max + 128) return false;                        // beyond any admissible amplicon (as k_pair)
					if(iloc + p_stop >= jloc - m_stop) return true;                      // pcr_assay.cpp:367-370
					int32_t amp_start = iloc + p_start;
					const int32_t amp_stop = min(jloc - m_start, L - 1);
					int32_t amp_len = amp_stop - amp_start + 1;
					if(amp_len < amp_min || amp_len > amp_max) return true;
					if(amp_start < 0){ amp_len += amp_start; amp_start = 0; }
					if(amp_len < 0 || amp_start + amp_len > L){ atomicOr(status, 1u); return true; }   // sequence.cpp:306 throw
					if(eos && has_split(planes, blk_base, amp_start, amp_len)) return true;
					best = fmaxf(best, identity(other, db[lo + (uint32_t)q].w, use_taq));
					return true;
				};
				if constexpr (WG_SEQ){
					const uint32_t *const cand = tb + other_bit*tw, *const strand = sb + (plus_role ? tw : 0u);
					const int32_t limit = amp_max + 128;
					if(plus_role){
						bool more = true;
						for(uint32_t wi = (k + 1u) >> 5;more && wi < tw && wi*32u < n;++wi){
							uint32_t bits = cand[wi] & strand[wi];
							if(wi == ((k + 1u) >> 5)) bits &= ~0u << ((k + 1u) & 31u);
							else if(((int32_t)(ls[wi*32u] & 0x7FFFFFFFu) - LOC_BIAS) - eloc > limit) break;   // the word's first entry is already beyond the window
							for(;bits;bits &= bits - 1){ if(!partner((int32_t)(wi*32u + (uint32_t)__ffs(bits) - 1u))){ more = false; break; } }
						}
					}
					else if(k > 0){
						bool more = true;
						for(int32_t wi = (int32_t)((k - 1u) >> 5);more && wi >= 0;--wi){
							uint32_t bits = cand[wi] & strand[wi];
							if(wi == (int32_t)((k - 1u) >> 5)) bits &= ~0u >> (31u - ((k - 1u) & 31u));
							else if(eloc - ((int32_t)(ls[min((uint32_t)wi*32u + 31u, n - 1u)] & 0x7FFFFFFFu) - LOC_BIAS) > limit) break;   // the word's last entry is already beyond
							for(;bits;){ const uint32_t hb = 31u - (uint32_t)__clz(bits); bits &= ~(1u << hb); if(!partner((int32_t)((uint32_t)wi*32u + hb))){ more = false; break; } }
						}
					}
				}
				else{
					for(int32_t q = plus_role ? (int32_t)k + 1 : (int32_t)k - 1;plus_role ? (q < (int32_t)n) : (q >= 0);q += plus_role ? 1 : -1){
						if(!((mw[q] >> other_bit) & 1u) || (ls[q] >> 31) != (plus_role ? 1u : 0u)){
							// (not a partner; the walk still ends with the window)
							const int32_t ploc = (int32_t)(ls[q] & 0x7FFFFFFFu) - LOC_BIAS;
							if((plus_role ? ploc - eloc : eloc - ploc) > amp_max + 128) break;
							continue;
						}
						if(!partner(q)) break;
					}
				}
				if(best < 0.0f) continue;                                                // no admissible amplicon through this entry
				const uint32_t slot = atomicAdd(&wg_n, 1u);
				if(slot < wg_cap){ MoveTask tk; tk.entry = e; tk.oligo_orient = o | ((uint32_t)orient << 31); tk.best = best; wg_tasks[slot] = tk; continue; }
				uint64_t *dst = (orient == 0) ? bits_fr : bits_rf;                        // the workgroup's list is full: in place
				const MoveJob job = jobs[o];
				const Planes ew = db[e].w;
				for(uint32_t v = job.v_begin;v < job.v_end;++v){
					const float var = identity(variants[v], ew, use_taq);
					const float f = (side == 0) ? var : best, r = (side == 0) ? best : var;
					if(sqrtf(__fmul_rn(f, r)) >= ident_thr)                         // pcr_assay.cpp:285-287
						atomicOr((unsigned long long *)&dst[(size_t)v*bit_words + (seq >> 6)], bit);
				}
			}
		}
		if constexpr (WG_SEQ){ if(w + 1u < mask_words) flush_tasks(); }              // (the last round's tasks leave through the common tail)
	}
	flush_tasks();
}

// One wave per task of k_pair_moves_batch (grid-stride; the task count is on the device): lane = trial word.
__global__ __launch_bounds__(256) void k_pair_moves_tasks(const MoveTask *__restrict__ tasks, const uint32_t *__restrict__ task_count, uint32_t task_cap,
	const DevEntry *__restrict__ db, const MoveJob *__restrict__ jobs, const OligoDev *__restrict__ variants, float ident_thr, int use_taq,
	uint64_t *__restrict__ bits_fr, uint64_t *__restrict__ bits_rf, uint64_t bit_words)
{
	const uint32_t n_tasks = min(task_count[0], task_cap);
	const uint32_t lane = threadIdx.x & 63u, wave = blockIdx.x*(blockDim.x >> 6) + (threadIdx.x >> 6), n_waves = gridDim.x*(blockDim.x >> 6);
	for(uint32_t k = wave;k < n_tasks;k += n_waves){
		const MoveTask t = tasks[k];
		const uint32_t o = t.oligo_orient & 0x7FFFFFFFu, orient = t.oligo_orient >> 31;
		const int side = (int)(o & 1u);
		const MoveJob job = jobs[o];
		const DevEntry ee = db[t.entry];
		uint64_t *dst = orient ? bits_rf : bits_fr;
		const uint64_t bit = 1ull << (ee.seq & 63);
		for(uint32_t v = job.v_begin + lane;v < job.v_end;v += 64){
			const float var = identity(variants[v], ee.w, use_taq);
			const float f = (side == 0) ? var : t.best, r = (side == 0) ? t.best : var;
			if(sqrtf(__fmul_rn(f, r)) >= ident_thr)                             // pcr_assay.cpp:285-287
				atomicOr((unsigned long long *)&dst[(size_t)v*bit_words + (ee.seq >> 6)], bit);
		}
	}
}

// compute_coverage's weight sum (pcr_assay.cpp:280-301) per trial word, in the reference's order: ascending sequence index
// over the {F(+),R(-)} bits, then over the {R(+),F(-)} bits not yet counted, accumulated in double (pcr_coverage_from_bits).
__global__ void k_cov_from_bits(const uint64_t *__restrict__ bits_fr, const uint64_t *__restrict__ bits_rf, uint64_t words, const float *__restrict__ weights,
	uint64_t n_seq, uint32_t n_variants, float *__restrict__ cov)
{
	const uint32_t v = blockIdx.x*blockDim.x + threadIdx.x;
	if(v >= n_variants) return;
	const uint64_t *fr = bits_fr + (size_t)v*words, *rf = bits_rf + (size_t)v*words;
	double ret = 0.0;
	for(uint64_t w = 0;w < words;++w){
		for(uint64_t m = fr[w];m;m &= m - 1){ const uint64_t i = w*64 + (uint64_t)(__ffsll((long long)m) - 1); if(i < n_seq) ret += weights[i]; }
	}
	for(uint64_t w = 0;w < words;++w){
		for(uint64_t m = rf[w] & ~fr[w];m;m &= m - 1){ const uint64_t i = w*64 + (uint64_t)(__ffsll((long long)m) - 1); if(i < n_seq) ret += weights[i]; }
	}
	cov[v] = (float)ret;
}

// k_key_coverage (pcr_multiplex.inc) for many assays: a thread owns one key of the multiplex background and walks the
// assays; the key counts for a trial word of (assay, side) when the OTHER oligo's map holds it at the threshold or the
// trial word's own identity reaches it (pcr_assay.cpp:304-336).
__global__ void k_key_coverage_batch(const Planes *__restrict__ keys, uint32_t n_keys, const OligoDev *__restrict__ base, uint32_t n_assays,
	const MoveJob *__restrict__ jobs, const OligoDev *__restrict__ variants, float thr, int use_taq, uint32_t *__restrict__ count)
{
	const uint32_t k = blockIdx.x*blockDim.x + threadIdx.x;
	if(k >= n_keys) return;
	const Planes key = keys[k];
	for(uint32_t a = 0;a < n_assays;++a){
		const OligoDev F = base[2*a], R = base[2*a + 1];
		const bool in_f = (uint32_t)__popc((key.a & F.m.a) | (key.c & F.m.c) | (key.g & F.m.g) | (key.t & F.m.t)) >= F.floor2;
		const bool in_r = (uint32_t)__popc((key.a & R.m.a) | (key.c & R.m.c) | (key.g & R.m.g) | (key.t & R.m.t)) >= R.floor2;
		if(!in_f && !in_r) continue;
		for(int side = 0;side < 2;++side){
			const MoveJob job = jobs[2*a + side];
			if(job.v_begin == job.v_end) continue;
			const bool in_edit = (side == 0) ? in_f : in_r, in_other = (side == 0) ? in_r : in_f;
			const bool other_ok = in_other && identity((side == 0) ? R : F, key, use_taq) >= thr;
			for(uint32_t v = job.v_begin;v < job.v_end;++v){
				if(other_ok || (in_edit && identity(variants[v], key, use_taq) >= thr)) atomicAdd(&count[v], 1u);
			}
		}
	}
}

// ------------------------------------------------------------------ Score (pcramp.h:158-208)
struct ScoreH { float tc, bc, ov; };
const ScoreH EMPTY_SCORE = {-1.0e6f, 1.0e6f, 0.0f};                             // Score(), pcramp.h:176-179
inline float accuracy(const ScoreH &s) { return s.tc - s.bc; }                  // pcramp.h:205
inline bool score_gt(const ScoreH &a, const ScoreH &b) { return (accuracy(a) == accuracy(b)) ? (a.ov > b.ov) : (accuracy(a) > accuracy(b)); }   // :190-197
inline bool score_lt(const ScoreH &a, const ScoreH &b) { return (accuracy(a) == accuracy(b)) ? (a.ov < b.ov) : (accuracy(a) < accuracy(b)); }   // :181-188
inline bool score_eq(const ScoreH &a, const ScoreH &b) { return accuracy(a) == accuracy(b) && a.ov == b.ov; }                                   // :199-203
inline float reuse_term(float v) { return (v == 1.0f) ? 10.0f : v; }            // MULTIPLEX_OLIGO_REUSE_BONUS, assay.h:19

struct TrialRow { Planes w; bool valid; float tc, bc, mc, pov; };

// One move function's loop over its trials (optimize_pcr.cpp): is_valid gate, coverage-bound shortcut (:95-109), Score
// comparison.  multiplex: the bound is `< 0`, the multiplex coverage joins the background term and the trial's reuse
// term is added -- increase_degeneracy alone never resets trial_score.oligo_overlap between its trials (:133-145), so
// there the maximum starts from the previous trial's total.
void decide_move(const TrialRow *rows, size_t n, const ScoreH &thr, int move, bool multiplex, float partial, Planes &best_w, ScoreH &best)
{
	best_w.a = best_w.c = best_w.g = best_w.t = 0; best = EMPTY_SCORE;
	float carried = 0.0f;
	for(size_t i = 0;i < n;++i){
		const TrialRow &r = rows[i];
		if(!r.valid) continue;
		const float bound = (r.tc + thr.bc) - thr.tc;
		if(multiplex ? (bound < 0.0f) : (bound <= 0.0f)) continue;
		ScoreH trial = {r.tc, r.bc, 0.0f};
		if(multiplex){
			trial.bc = r.bc + r.mc;
			float ov = (move == PCR_MOVE_INCREASE_DEGENERACY) ? std::max(r.pov, carried) : r.pov;
			ov = reuse_term(ov) + partial;
			carried = ov; trial.ov = ov;
		}
		if(score_gt(trial, best)){ best = trial; best_w = r.w; }
	}
}

inline bool planes_eq(const Planes &x, const Planes &y) { return x.a == y.a && x.c == y.c && x.g == y.g && x.t == y.t; }
inline pcr_word128 word_of(const Planes &p) { pcr_word128 w; pcrhost::word_of_planes(p, w.w); return w; }

struct PoolPlanes { std::vector<Planes> pp; };
inline float pool_overlap(const Planes &w, const PoolPlanes &P)
{
	float best = 0.0f;
	for(const Planes &p : P.pp) best = std::max(best, pcrhost::max_overlap(w, p));
	return best;
}

// what one iteration evaluates for one assay
struct IterAssay {
	Planes f, r;
	std::vector<TrialRow> rows[2];                       // per side, all moves in order
	std::vector<std::pair<uint32_t, uint32_t> > span[2]; // per side and move: [begin, end) into rows
	ScoreH base;                                          // Score of the unmodified assay
};

// The move-coverage bitsets of one sequence set for all assays of the iteration, enqueued on the handle's stream: variant 0 of
// (assay, side 0) is the assay's own forward oligo (the base Score), the valid trial words follow.  *words_out = bitset words per
// variant in ctx->bits_fr / bits_rf (0: the set has no DB entries or there are no variants -- every coverage is 0); the has_split
// flag of the pass is in ctx->status.
int coverage_bits(pcr_ctx *ctx, SeqSet &S, const std::vector<OligoDev> &base, const std::vector<MoveJob> &jobs, const std::vector<OligoDev> &variants,
	const pcr_amplify_args &a, uint64_t *words_out)
{
	*words_out = 0;
	const uint32_t nv = (uint32_t)variants.size();
	if(!S.have_db){ g_err = "pcr_optimize_batch: no word DB (call pcr_select_words on the set first)"; return PCR_ERR_STATE; }
	{ const int erc = ensure_touched(ctx, S); if(erc != PCR_OK) return erc; }
	if(S.n_entries == 0 || nv == 0) return PCR_OK;
	int rc;
	const uint32_t n_oligo = (uint32_t)base.size(), mask_words = (n_oligo + 31)/32;
	const uint64_t words = (S.n + 63)/64;
	const size_t total = (size_t)nv*words;
	if((rc = ctx->bits_fr.ensure(total + 2)) != PCR_OK) return rc;
	if((rc = ctx->bits_rf.ensure(total + 2)) != PCR_OK) return rc;
	if((rc = ctx->mask.ensure((size_t)S.n_slots*mask_words)) != PCR_OK) return rc;
	if((rc = ctx->status.ensure(1)) != PCR_OK) return rc;
	if((rc = ctx->opt_oligos.ensure(base.size() + variants.size() + 2)) != PCR_OK) return rc;
	if((rc = ctx->opt_jobs.ensure(jobs.size() + 1)) != PCR_OK) return rc;
	if((rc = ctx->opt_cov.ensure((size_t)nv + 4)) != PCR_OK) return rc;
	if(S.d_weight.cap < S.n || S.weight_dirty){
		if((rc = S.d_weight.ensure(S.n + 1)) != PCR_OK) return rc;
		HIP_TRY(hipMemcpyAsync(S.d_weight.p, S.weight.data(), S.n*sizeof(float), hipMemcpyHostToDevice, ctx->stream));
		S.weight_dirty = false;
	}
	HIP_TRY(hipMemcpyAsync(ctx->opt_oligos.p, base.data(), base.size()*sizeof(OligoDev), hipMemcpyHostToDevice, ctx->stream));
	HIP_TRY(hipMemcpyAsync(ctx->opt_oligos.p + base.size(), variants.data(), variants.size()*sizeof(OligoDev), hipMemcpyHostToDevice, ctx->stream));
	HIP_TRY(hipMemcpyAsync((void *)ctx->opt_jobs.p, jobs.data(), jobs.size()*sizeof(MoveJob), hipMemcpyHostToDevice, ctx->stream));
	HIP_TRY(hipMemsetAsync(ctx->bits_fr.p, 0, total*sizeof(uint64_t), ctx->stream));
	HIP_TRY(hipMemsetAsync(ctx->bits_rf.p, 0, total*sizeof(uint64_t), ctx->stream));
	const uint32_t n_db = S.n_touched*S.db_cap;
	if((rc = ctx->opt_loc.ensure((size_t)S.n_slots + 1)) != PCR_OK) return rc;
	if(n_oligo <= 32)
		hipLaunchKernelGGL(k_match_few_t, dim3((n_db + 255)/256), dim3(256), 0, ctx->stream, S.db.p, n_db, S.db_cap, S.touched.p, S.d_seg_hi, ctx->opt_oligos.p, n_oligo,
			ctx->mask.p, ctx->opt_loc.p, ctx->status.p);
	else
		hipLaunchKernelGGL(k_match_t, dim3(std::max(1u, (S.n_touched + MATCH_WAVES - 1)/MATCH_WAVES)), dim3(64*MATCH_WAVES), 0, ctx->stream, S.db.p, S.n_touched, S.db_cap,
			S.touched.p, S.d_seg_hi, ctx->opt_oligos.p, n_oligo, mask_words, (uint64_t)S.n_slots, ctx->mask.p, ctx->opt_loc.p, ctx->status.p);
	HIP_TRY(hipGetLastError());
	uint32_t task_cap = (uint32_t)std::min<uint64_t>(std::max<uint64_t>((uint64_t)n_db*4, 1u << 16), 1u << 26);
	if(ctx->opt_dbg_task_cap) task_cap = std::min(task_cap, ctx->opt_dbg_task_cap);      // test hook: make the global list overflow
	const uint32_t wg_cap = ctx->opt_dbg_wg_tasks ? std::min(ctx->opt_dbg_wg_tasks, PM_WG_TASKS) : PM_WG_TASKS;
	if((rc = ctx->opt_tasks.ensure((size_t)task_cap*3 + 4)) != PCR_OK) return rc;   // MoveTask = 3 words; the count sits behind them
	uint32_t *const d_task_count = ctx->opt_tasks.p + (size_t)task_cap*3;
	HIP_TRY(hipMemsetAsync(d_task_count, 0, sizeof(uint32_t), ctx->stream));
#define PM_ARGS S.db_cap, S.touched.p, S.d_seg_hi, ctx->mask.p, ctx->opt_loc.p, \
		mask_words, (uint64_t)S.n_slots, ctx->opt_oligos.p, n_oligo, (const MoveJob *)ctx->opt_jobs.p, ctx->opt_oligos.p + base.size(), S.planes.p, S.d_blk_off.p, S.d_len.p, \
		S.d_active.p, S.d_has_eos.p, a.amp_min, a.amp_max, a.ident_threshold, a.use_taq_mama, ctx->bits_fr.p, ctx->bits_rf.p, words, ctx->status.p, \
		(MoveTask *)ctx->opt_tasks.p, d_task_count, task_cap, wg_cap
	// a sequence's (position | strand) words and one mask word of each of its entries live in LDS while its partners are walked:
	// a wave per sequence while the buckets hold at most 64 entries, a workgroup per sequence up to 4 096 (52 KB of LDS); beyond that the global walk
	if(ctx->opt_pm_global || S.db_cap > 4096u)
		hipLaunchKernelGGL(k_pair_moves_batch, dim3((n_db + PM_THREADS - 1)/PM_THREADS), dim3(PM_THREADS), 0, ctx->stream, S.db.p, n_db, PM_ARGS);
	else if(S.db_cap <= 64u)
		hipLaunchKernelGGL(k_pair_moves_lds<false>, dim3((S.n_touched + 3)/4), dim3(256), 4*2*64*sizeof(uint32_t), ctx->stream, S.db.p, S.n_touched, PM_ARGS);
	else
		hipLaunchKernelGGL(k_pair_moves_lds<true>, dim3(S.n_touched), dim3(256), (2*(size_t)S.db_cap + 34*(((size_t)S.db_cap + 31)/32))*sizeof(uint32_t), ctx->stream, S.db.p, S.n_touched, PM_ARGS);
#undef PM_ARGS
	HIP_TRY(hipGetLastError());
	hipLaunchKernelGGL(k_pair_moves_tasks, dim3(ctx->n_cu*8), dim3(256), 0, ctx->stream, (const MoveTask *)ctx->opt_tasks.p, d_task_count, task_cap, S.db.p,
		(const MoveJob *)ctx->opt_jobs.p, ctx->opt_oligos.p + base.size(), a.ident_threshold, a.use_taq_mama, ctx->bits_fr.p, ctx->bits_rf.p, words);
	HIP_TRY(hipGetLastError());
	*words_out = words;
	return PCR_OK;
}

// The coverage pass of one sequence set: cov_out[v] for the flat variant list (coverage_bits + compute_coverage's sum).
int coverage_pass(pcr_ctx *ctx, SeqSet &S, const std::vector<OligoDev> &base, const std::vector<MoveJob> &jobs, const std::vector<OligoDev> &variants,
	const pcr_amplify_args &a, std::vector<float> &cov_out)
{
	const uint32_t nv = (uint32_t)variants.size();
	cov_out.assign(nv, 0.0f);
	uint64_t words = 0;
	const int rc = coverage_bits(ctx, S, base, jobs, variants, a, &words);
	if(rc != PCR_OK || words == 0) return rc;
	hipLaunchKernelGGL(k_cov_from_bits, dim3((nv + 127)/128), dim3(128), 0, ctx->stream, ctx->bits_fr.p, ctx->bits_rf.p, words, S.d_weight.p, (uint64_t)S.n, nv, ctx->opt_cov.p);
	HIP_TRY(hipGetLastError());
	uint32_t status = 0;
	HIP_TRY(hipMemcpyAsync(cov_out.data(), ctx->opt_cov.p, (size_t)nv*sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
	HIP_TRY(hipMemcpyAsync(&status, ctx->status.p, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
	HIP_TRY(hipStreamSynchronize(ctx->stream));
	if(status & 1u){ g_err = "Sequence::has_split: range is out of bounds"; return PCR_ERR_RANGE; }   // sequence.cpp:306-308
	return PCR_OK;
}

// The target pass of a sharded iteration (pcr_shard.inc): the header agreement (local_rc: what this rank met earlier in the
// iteration), this rank's bitsets, the combine over the ranks.  `late` runs while the bitsets are computed (the thermodynamics'
// verdicts); its outcome travels in the combine's status word.  Every rank returns the same code.
int coverage_pass_sharded(pcr_ctx *ctx, SeqSet &S, const std::vector<OligoDev> &base, const std::vector<MoveJob> &jobs, const std::vector<OligoDev> &variants,
	const pcr_amplify_args &a, std::vector<float> &cov_out, int local_rc, const std::function<int()> &late)
{
	const uint32_t nv = (uint32_t)variants.size();
	cov_out.assign(nv, 0.0f);
	const int rc = shard_header(ctx, local_rc, nv, sh_hash(SH_HASH0, jobs.data(), jobs.size()*sizeof(MoveJob)));
	if(rc != PCR_OK) return rc;
	if(nv == 0) return late();                                                     // (an assay always has its base word: not reached)
	uint64_t words = 0;
	const int brc = coverage_bits(ctx, S, base, jobs, variants, a, &words);
	const int lrc = late();
	return shard_combine(ctx, S, nv, words, words != 0, brc != PCR_OK ? brc : lrc, cov_out);
}

int multiplex_pass(pcr_ctx *ctx, const std::vector<OligoDev> &base, const std::vector<MoveJob> &jobs, const std::vector<OligoDev> &variants,
	float thr, int use_taq, std::vector<float> &cov_out)
{
	const uint32_t nv = (uint32_t)variants.size();
	cov_out.assign(nv, 0.0f);
	if(ctx->mx_n_keys == 0 || nv == 0) return PCR_OK;                            // pcr_assay.cpp:75-77, :306-308
	int rc;
	if((rc = ctx->opt_oligos.ensure(base.size() + variants.size() + 2)) != PCR_OK) return rc;
	if((rc = ctx->opt_jobs.ensure(jobs.size() + 1)) != PCR_OK) return rc;
	if((rc = ctx->mx_count.ensure((size_t)nv + 4)) != PCR_OK) return rc;
	HIP_TRY(hipMemcpyAsync(ctx->opt_oligos.p, base.data(), base.size()*sizeof(OligoDev), hipMemcpyHostToDevice, ctx->stream));
	HIP_TRY(hipMemcpyAsync(ctx->opt_oligos.p + base.size(), variants.data(), variants.size()*sizeof(OligoDev), hipMemcpyHostToDevice, ctx->stream));
	HIP_TRY(hipMemcpyAsync((void *)ctx->opt_jobs.p, jobs.data(), jobs.size()*sizeof(MoveJob), hipMemcpyHostToDevice, ctx->stream));
	HIP_TRY(hipMemsetAsync(ctx->mx_count.p, 0, (size_t)nv*sizeof(uint32_t), ctx->stream));
	hipLaunchKernelGGL(k_key_coverage_batch, dim3((ctx->mx_n_keys + 255)/256), dim3(256), 0, ctx->stream, ctx->mx_keys.p, ctx->mx_n_keys, ctx->opt_oligos.p,
		(uint32_t)(base.size()/2), (const MoveJob *)ctx->opt_jobs.p, ctx->opt_oligos.p + base.size(), thr, use_taq, ctx->mx_count.p);
	HIP_TRY(hipGetLastError());
	std::vector<uint32_t> cnt(nv);
	HIP_TRY(hipMemcpyAsync(cnt.data(), ctx->mx_count.p, (size_t)nv*sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
	HIP_TRY(hipStreamSynchronize(ctx->stream));
	for(uint32_t v = 0;v < nv;++v) cov_out[v] = (float)(double)cnt[v];            // "each multiplex background gets weight 1.0", summed in double
	return PCR_OK;
}

// Everything one optimiser iteration needs for the listed assays: trial words, is_valid, the three coverages, pool overlaps.
// only_side / only_move >= 0 restrict the trials (pcr_optimization_move).
double g_opt_t[6] = {0, 0, 0, 0, 0, 0};     // PCRAMP_TIMING=1: trials | thermo | variant lists | target pass | background pass | multiplex + scatter (ms)
struct OptTimer {
	bool on; int slot; std::chrono::steady_clock::time_point t0;
	explicit OptTimer(bool o) : on(o), slot(0) { if(on) t0 = std::chrono::steady_clock::now(); }
	void next(int s2){ if(!on) return; const auto t1 = std::chrono::steady_clock::now(); g_opt_t[slot] += std::chrono::duration<double, std::milli>(t1 - t0).count(); slot = s2; t0 = t1; }
	~OptTimer(){ next(slot); }
};

// Host-side loops over independent assays on a few threads (the GPU box gives a process 16 cores): part p of n_parts takes the
// assays [part_end(p - 1), part_end(p)); the parts' outputs are joined in part order, so the result does not depend on which thread
// ran which.  The threads are the handle's (HostPool, pcr_device.hip), started once: an optimiser call runs ~30 of these loops and a
// std::thread per part and loop was a third of the loops' 10 ms.  Small batches stay on the calling thread.
inline unsigned host_parts(pcr_ctx *ctx, uint32_t n)
{
	if(n < 32) return 1;
	return std::min<unsigned>(ctx->host_pool().size() + 1u, n/16u);
}
inline uint32_t part_end(uint32_t n, unsigned n_parts, unsigned part) { return (uint32_t)(((uint64_t)n*(part + 1u))/n_parts); }
template<class F> void for_ranges(pcr_ctx *ctx, uint32_t n, unsigned n_parts, F f /* (lo, hi, part) */)
{
	if(n_parts <= 1){ f(0u, n, 0u); return; }
	ctx->host_pool().run(n_parts, [&f, n, n_parts](unsigned p){ f(p ? part_end(n, n_parts, p - 1) : 0u, part_end(n, n_parts, p), p); });
}

// is_valid of the trial words met so far in this call (the thermodynamic options are fixed within a call): from one iteration
// to the next only one oligo of an assay changes, so the trial words of the other recur.
// (An open-addressing table in one allocation: with hundreds of thousands of words per call a node-based map spent more time
// in malloc than the thermodynamics kernel took, the more so once the process has threads.)
struct ValidCache {
	struct Slot { uint32_t a, c, g, t; int32_t v; };                            // v: -1 empty, 0 / 1 = is_valid
	std::vector<Slot> tab; size_t used = 0;
	static size_t hash(const Planes &w)
	{
		uint64_t h = ((uint64_t)w.a << 32 | w.c)*0x9E3779B97F4A7C15ull;
		h ^= ((uint64_t)w.g << 32 | w.t)*0xC2B2AE3D27D4EB4Full; h ^= h >> 29; h *= 0x165667B19E3779F9ull; h ^= h >> 32;
		return (size_t)h;
	}
	int find(const Planes &w) const                                               // -1: not there
	{
		if(tab.empty()) return -1;
		const size_t mask = tab.size() - 1;
		for(size_t i = hash(w) & mask;;i = (i + 1) & mask){
			const Slot &s = tab[i];
			if(s.v < 0) return -1;
			if(s.a == w.a && s.c == w.c && s.g == w.g && s.t == w.t) return s.v;
		}
	}
	void put(const Planes &w, bool ok)
	{
		if((used + 1)*10 >= tab.size()*6) grow();
		const size_t mask = tab.size() - 1;
		for(size_t i = hash(w) & mask;;i = (i + 1) & mask){
			Slot &s = tab[i];
			if(s.v < 0){ s.a = w.a; s.c = w.c; s.g = w.g; s.t = w.t; s.v = ok ? 1 : 0; ++used; return; }
			if(s.a == w.a && s.c == w.c && s.g == w.g && s.t == w.t){ s.v = ok ? 1 : 0; return; }
		}
	}
	void grow()
	{
		std::vector<Slot> old; old.swap(tab);
		const Slot empty = {0u, 0u, 0u, 0u, -1};
		tab.assign(std::max<size_t>(old.size()*2, size_t(1) << 16), empty);
		used = 0;
		for(const Slot &s : old){ if(s.v >= 0){ const Planes w = {s.a, s.c, s.g, s.t}; put(w, s.v != 0); } }
	}
};

int evaluate_iteration(pcr_ctx *ctx, std::vector<IterAssay> &A, const pcr_optimize_args *o, const PoolPlanes *pool, int only_side, int only_move,
	ValidCache *vc = nullptr)
{
	OptTimer timer(ctx->timing);
	const bool multiplex = pool != nullptr;
	const uint32_t n = (uint32_t)A.size();
	// sharded (pcr_shard.inc): a failure before the target combine is reported to the other ranks at its header step
	const bool sharded = ctx->shard_comm != nullptr;
	auto fail = [&](int rc) -> int { return sharded ? shard_header(ctx, rc, 0, 0) : rc; };
	// ---- trial words and their is_valid jobs.  The assays are independent: ranges of them go to a few host threads (1 000
	// trial assays make ~200 000 trial words per iteration), whose lists are then joined in assay order.
	std::vector<thermo::Job> tj;                                                  // one packed record per trial word that needs thermodynamics
	std::vector<uint32_t> n_exp;                                                  // its number of IUPAC expansions (the device spells them)
	std::vector<uint32_t> first;                                                  // per trial word: its record (or the next one's, if it has none)
	std::vector<int8_t> known;                                                    // per trial word: is_valid from the cache (0 / 1) or -1
	{
		struct Part { std::vector<thermo::Job> tj; std::vector<uint32_t> n_exp, first; std::vector<int8_t> known; int err = 0; };
		const unsigned n_parts = host_parts(ctx, n);
		std::vector<Part> parts(n_parts);
		for_ranges(ctx, n, n_parts, [&](uint32_t lo, uint32_t hi, unsigned part){
			Part &P = parts[part];
			std::vector<Planes> tmp;
			for(uint32_t a = lo;a < hi && !P.err;++a){
				for(int side = 0;side < 2 && !P.err;++side){
					A[a].rows[side].clear(); A[a].span[side].assign((size_t)o->n_moves, std::make_pair(0u, 0u));
					if(only_side >= 0 && side != only_side) continue;
					for(int k = 0;k < o->n_moves && !P.err;++k){
						const int mv = o->moves[k];
						if(only_move >= 0 && mv != only_move) continue;
						tmp.clear();
						if(!pcrhost::move_trials(side ? A[a].r : A[a].f, mv, o->max_degen, o->primer_min, o->primer_max, tmp)){ P.err = 1; break; }
						const uint32_t b = (uint32_t)A[a].rows[side].size();
						for(const Planes &w : tmp){
							TrialRow r; r.w = w; r.valid = false; r.tc = r.bc = r.mc = r.pov = 0.0f;
							A[a].rows[side].push_back(r);
							P.first.push_back((uint32_t)P.tj.size());
							if(vc){
								const int v = vc->find(w);                                 // (read-only here: the cache is written after the thermodynamics)
								P.known.push_back((int8_t)v);
								if(v >= 0) continue;
							}
							else P.known.push_back(-1);
							if(!pcrhost::planes_occupied(w) || !append_valid_record(w, &o->thermo, P.tj, P.n_exp)){ P.err = 2; break; }
						}
						A[a].span[side][(size_t)k] = std::make_pair(b, (uint32_t)A[a].rows[side].size());
					}
				}
			}
		});
		for(const Part &P : parts){
			if(P.err == 1){ g_err = "pcr_optimize_batch: unknown move"; return fail(PCR_ERR_ARG); }
			if(P.err == 2){ g_err = "pcr_optimize_batch: a trial oligo is longer than 32, holds a non-base slot or has more than 65536 expansions"; return fail(PCR_ERR_ARG); }
		}
		for(const Part &P : parts){
			const uint32_t off = (uint32_t)tj.size();
			tj.insert(tj.end(), P.tj.begin(), P.tj.end());
			n_exp.insert(n_exp.end(), P.n_exp.begin(), P.n_exp.end());
			known.insert(known.end(), P.known.begin(), P.known.end());
			for(uint32_t f : P.first) first.push_back(f + off);
		}
	}
	first.push_back((uint32_t)tj.size());
	timer.next(1);
	if(ctx->timing && getenv("PCRAMP_TIMING_ITER")) fprintf(stderr, "[pcramp] iteration: %u assays, %zu trial words, %zu thermo records\n", n, known.size(), tj.size());
	// ---- is_valid of the trial words the cache does not know: on a host thread and a stream of their own, BESIDE the coverage passes
	// below.  Coverage does not depend on validity -- it only is not needed for an invalid word -- so the passes take every word that
	// is not known to be invalid, and the verdicts are applied afterwards.  (One after the other, the thermodynamics were 13.5 of an
	// optimize_batch call's 50 ms at 256 assays, most of it host work around a 0.2 ms kernel: records, the expansion map, copies.)
	std::vector<uint8_t> bad;
	int rc = PCR_OK, rc_th = PCR_OK;
	std::string err_th;
	std::thread th_thread;
	bool beside = !tj.empty() && !getenv("PCRAMP_OPT_SERIAL");
	if(beside){
		hipError_t e = hipSuccess;
		if(!ctx->aux_stream) e = ctx->aux_stream.create(hipStreamNonBlocking);
		if(e == hipSuccess) e = hipStreamSynchronize(ctx->stream);               // (nothing of this handle is in flight that the records could race with)
		if(e != hipSuccess){ g_err = std::string("pcr_optimize_batch: ") + hipGetErrorString(e); return fail(PCR_ERR_DEVICE); }
		try{
			th_thread = std::thread([&]{
				if(hipSetDevice(ctx->device) != hipSuccess){ rc_th = PCR_ERR_DEVICE; err_th = "hipSetDevice failed on the thermodynamics thread"; return; }
				rc_th = run_thermo_valid(ctx, tj, n_exp, &o->thermo, bad, ctx->aux_stream);
				if(rc_th != PCR_OK) err_th = g_err;
			});
		}
		catch(const std::exception &){                                                // no thread to be had: one after the other, as below
			beside = false;
			rc = run_thermo_valid(ctx, tj, n_exp, &o->thermo, bad);
			if(rc != PCR_OK) return fail(rc);
		}
	}
	else{
		rc = run_thermo_valid(ctx, tj, n_exp, &o->thermo, bad);
		if(rc != PCR_OK) return fail(rc);
	}
	struct Joiner { std::thread &t; ~Joiner(){ if(t.joinable()) t.join(); } } joiner{th_thread};   // every return path waits for the thread
	auto apply_verdicts = [&](){
		size_t t = 0;
		for(uint32_t a = 0;a < n;++a) for(int side = 0;side < 2;++side) for(TrialRow &r : A[a].rows[side]){
			bool ok = true;
			if(known[t] >= 0) ok = known[t] != 0;
			else{
				for(uint32_t k = first[t];k < first[t + 1];++k){ if(bad[k]) ok = false; }      // valid_pcr.cpp:19-31, every expansion (run_thermo_valid)
				if(vc) vc->put(r.w, ok);
			}
			r.valid = ok; ++t;
		}
	};
	{
		// until the verdicts are in, `valid` means "takes part in the coverage passes": known valid, or not known yet
		size_t t = 0;
		for(uint32_t a = 0;a < n;++a) for(int side = 0;side < 2;++side) for(TrialRow &r : A[a].rows[side]) r.valid = (known[t++] != 0);
		if(!beside) apply_verdicts();
	}
	timer.next(2);
	// ---- flat variant lists: per (assay, side) the valid trial words; (assay, side 0) starts with the assay's own F (base Score)
	std::vector<OligoDev> base_t(2*(size_t)n), base_b(2*(size_t)n), base_m(2*(size_t)n), var_t, var_b, var_m;
	std::vector<MoveJob> jobs(2*(size_t)n);
	const float t2 = o->target.collect_threshold*o->target.collect_threshold, b2 = o->background.collect_threshold*o->background.collect_threshold;
	const bool want_b = o->have_background != 0;
	{
		struct Part { std::vector<OligoDev> t, b, m; };
		const unsigned n_parts = host_parts(ctx, n);
		std::vector<Part> parts(n_parts);
		for_ranges(ctx, n, n_parts, [&](uint32_t lo, uint32_t hi, unsigned part){
			Part &P = parts[part];
			auto push = [&](const Planes &w){
				OligoDev d; fill_oligo_planes(d, w, t2); P.t.push_back(d);               // the three tables differ in the floor only (optimize.cpp:293)
				if(!want_b && !multiplex) return;
				const float size = (float)(unsigned)pcrhost::planes_size(d.m);
				if(want_b){ d.floor2 = (unsigned)(size*b2); P.b.push_back(d); }
				if(multiplex){ d.floor2 = (unsigned)(size*o->multiplex_threshold); P.m.push_back(d); }   // match_words at background_threshold, NOT squared (pcr_assay.cpp:86,96)
			};
			for(uint32_t a = lo;a < hi;++a){
				const pcr_word128 wf = word_of(A[a].f), wr = word_of(A[a].r);
				fill_oligo(base_t[2*a], wf.w, t2); fill_oligo(base_t[2*a + 1], wr.w, t2);
				fill_oligo(base_b[2*a], wf.w, b2); fill_oligo(base_b[2*a + 1], wr.w, b2);
				fill_oligo(base_m[2*a], wf.w, o->multiplex_threshold); fill_oligo(base_m[2*a + 1], wr.w, o->multiplex_threshold);
				for(int side = 0;side < 2;++side){
					jobs[2*a + side].v_begin = (uint32_t)P.t.size();                    // relative to the part; shifted when the parts are joined
					if(side == 0) push(A[a].f);
					for(const TrialRow &r : A[a].rows[side]){ if(r.valid) push(r.w); }
					jobs[2*a + side].v_end = (uint32_t)P.t.size();
				}
			}
		});
		uint32_t lo = 0;
		for(unsigned part = 0;part < n_parts;++part){
			const uint32_t hi = part_end(n, n_parts, part), off = (uint32_t)var_t.size();
			for(uint32_t a = lo;a < hi;++a) for(int side = 0;side < 2;++side){ jobs[2*a + side].v_begin += off; jobs[2*a + side].v_end += off; }
			var_t.insert(var_t.end(), parts[part].t.begin(), parts[part].t.end());
			var_b.insert(var_b.end(), parts[part].b.begin(), parts[part].b.end());
			var_m.insert(var_m.end(), parts[part].m.begin(), parts[part].m.end());
			lo = hi;
		}
	}
	std::vector<float> tcov, bcov, mcov;
	std::vector<uint8_t> took;                                                    // per trial word: it has a slot in the variant lists
	auto join_verdicts = [&]() -> int {
		for(uint32_t a = 0;a < n;++a) for(int side = 0;side < 2;++side) for(const TrialRow &r : A[a].rows[side]) took.push_back(r.valid ? 1 : 0);
		th_thread.join();
		if(rc_th != PCR_OK){ g_err = err_th; return rc_th; }
		apply_verdicts();
		return PCR_OK;
	};
	timer.next(3);
	if(sharded){
		// everything local first -- background and multiplex passes beside the thermodynamics -- so that the target combine's
		// header carries the failures of the iteration, and the verdicts' (joined while the target bitsets are computed) its
		// status word: after the header, no rank can leave on its own
		int lrc = PCR_OK;
		if(o->have_background) lrc = coverage_pass(ctx, ctx->sets[PCR_SET_BACKGROUND], base_b, jobs, var_b, o->background, bcov);
		else bcov.assign(var_t.size(), 0.0f);
		if(lrc == PCR_OK){
			if(multiplex) lrc = multiplex_pass(ctx, base_m, jobs, var_m, o->multiplex_threshold, o->target.use_taq_mama, mcov);
			else mcov.assign(var_t.size(), 0.0f);
		}
		timer.next(4);
		if((rc = coverage_pass_sharded(ctx, ctx->sets[PCR_SET_TARGET], base_t, jobs, var_t, o->target, tcov, lrc,
			[&]() -> int { return beside ? join_verdicts() : PCR_OK; })) != PCR_OK) return rc;
		timer.next(5);
	}
	else{
		if((rc = coverage_pass(ctx, ctx->sets[PCR_SET_TARGET], base_t, jobs, var_t, o->target, tcov)) != PCR_OK) return rc;
		timer.next(4);
		if(o->have_background){ if((rc = coverage_pass(ctx, ctx->sets[PCR_SET_BACKGROUND], base_b, jobs, var_b, o->background, bcov)) != PCR_OK) return rc; }
		else bcov.assign(var_t.size(), 0.0f);
		timer.next(5);
		if(multiplex){ if((rc = multiplex_pass(ctx, base_m, jobs, var_m, o->multiplex_threshold, o->target.use_taq_mama, mcov)) != PCR_OK) return rc; }
		else mcov.assign(var_t.size(), 0.0f);
		if(beside){ if((rc = join_verdicts()) != PCR_OK) return rc; }
	}
	size_t tk = 0;
	for(uint32_t a = 0;a < n;++a){
		for(int side = 0;side < 2;++side){
			uint32_t v = jobs[2*a + side].v_begin;
			if(side == 0){
				// Score of the unmodified assay (optimize.cpp:72-97)
				A[a].base.tc = tcov[v]; A[a].base.bc = multiplex ? (bcov[v] + mcov[v]) : bcov[v];
				A[a].base.ov = multiplex ? pcrhost::oligo_overlap(A[a].f, A[a].r, pool->pp.data(), (uint32_t)(pool->pp.size()/2)) : 0.0f;
				++v;
			}
			for(TrialRow &r : A[a].rows[side]){
				const bool has_slot = beside ? (took[tk++] != 0) : r.valid;
				if(!has_slot) continue;
				if(r.valid){
					r.tc = tcov[v]; r.bc = bcov[v]; r.mc = mcov[v];
					r.pov = multiplex ? pool_overlap(r.w, *pool) : 0.0f;
				}
				++v;
			}
		}
	}
	return PCR_OK;
}

bool check_opt_args(const pcr_optimize_args *o)
{
	if(!o || o->n_moves < 0 || o->n_moves > 8) return false;
	for(int k = 0;k < o->n_moves;++k){ if(o->moves[k] < 0 || o->moves[k] > PCR_MOVE_GROW3) return false; }
	return true;
}

} // namespace

extern "C" {

int pcr_optimize_batch(pcr_ctx *ctx, const pcr_pair *assays, uint32_t n, const pcr_optimize_args *o, const pcr_pair *pool, uint32_t n_pool,
	pcr_pair *best_out, float *score_out, uint32_t *iterations_out)
{
	if(!ctx){ g_err = "pcr_optimize_batch: bad argument"; return PCR_ERR_ARG; }
	const bool args_ok = check_opt_args(o) && !(n && (!assays || !best_out)) && !(n_pool && !pool);
	if(!args_ok) g_err = "pcr_optimize_batch: bad argument";
	if(ctx->shard_comm){                                                           // sharded: every rank enters with the same call, or none goes on
		int rc0 = args_ok ? enter_device(ctx) : PCR_ERR_ARG;
		rc0 = shard_agree(ctx, rc0 == PCR_OK ? opt_fingerprint(1, assays, n, o, pool, n_pool) : 0, rc0, "pcr_optimize_batch");
		if(rc0 != PCR_OK) return rc0;
	}
	if(!args_ok) return PCR_ERR_ARG;
	DRAIN(ctx);
	HIP_TRY(hipSetDevice(ctx->device));
	const bool multiplex = o->use_multiplex != 0;
	PoolPlanes P;
	if(multiplex){ for(uint32_t i = 0;i < n_pool;++i){ P.pp.push_back(pcrhost::planes_of_word(pool[i].f.w)); P.pp.push_back(pcrhost::planes_of_word(pool[i].r.w)); } }
	struct State { Planes f, r, best_f, best_r; ScoreH best; bool live; uint32_t iters; std::vector<std::pair<Planes, Planes> > previous; };
	std::vector<State> st(n);
	for(uint32_t i = 0;i < n;++i){
		st[i].f = st[i].best_f = pcrhost::planes_of_word(assays[i].f.w); st[i].r = st[i].best_r = pcrhost::planes_of_word(assays[i].r.w);
		st[i].best = EMPTY_SCORE; st[i].live = true; st[i].iters = 0;
		st[i].previous.push_back(std::make_pair(st[i].f, st[i].r));
	}
	std::vector<IterAssay> A;
	std::vector<uint32_t> who;
	ValidCache valid_cache;
	while(true){
		A.clear(); who.clear();
		for(uint32_t i = 0;i < n;++i){ if(st[i].live){ IterAssay x; x.f = st[i].f; x.r = st[i].r; A.push_back(x); who.push_back(i); } }
		if(A.empty()) break;
		const int rc = evaluate_iteration(ctx, A, o, multiplex ? &P : nullptr, -1, -1, &valid_cache);
		if(rc != PCR_OK) return rc;
		for(size_t k = 0;k < A.size();++k){
			State &s = st[who[k]];
			const IterAssay &x = A[k];
			++s.iters;
			const ScoreH approx = x.base;
			if(score_lt(approx, s.best)){ s.live = false; continue; }             // optimize.cpp:99-103: the last step made it worse
			s.best = approx; s.best_f = s.f; s.best_r = s.r;
			// every move of every oligo against the running best (optimize.cpp:120-140): `local_score` doubles as the moves'
			// score threshold, ties go to the lower degeneracy (:133-135)
			Planes local_seq; local_seq.a = local_seq.c = local_seq.g = local_seq.t = 0;
			int local_oligo = -1; ScoreH local = approx; bool improved = false;
			for(int side = 0;side < 2;++side){
				const float partial = multiplex ? reuse_term(pool_overlap(side ? s.f : s.r, P)) : 0.0f;   // the other oligo's reuse term (optimize_pcr.cpp:27-53)
				for(int m = 0;m < o->n_moves;++m){
					const std::pair<uint32_t, uint32_t> sp = x.span[side][(size_t)m];
					Planes w; ScoreH sc;
					decide_move(x.rows[side].data() + sp.first, sp.second - sp.first, local, o->moves[m], multiplex, partial, w, sc);
					if(score_gt(sc, local) || (score_eq(sc, local) && pcrhost::planes_degeneracy(w) < pcrhost::planes_degeneracy(local_seq))){
						local = sc; local_seq = w; local_oligo = side; improved = true;
					}
				}
			}
			if(!improved){ s.live = false; continue; }
			const Planes centred = planes_center(local_seq);                       // optimize.cpp:152
			if(local_oligo == 0) s.f = centred; else s.r = centred;
			bool seen = false;
			for(const std::pair<Planes, Planes> &p : s.previous){ if(planes_eq(p.first, s.f) && planes_eq(p.second, s.r)){ seen = true; break; } }   // :196-202
			if(seen){ s.live = false; continue; }
			s.previous.push_back(std::make_pair(s.f, s.r));
		}
	}
	if(ctx->timing) fprintf(stderr, "[pcramp] optimize_batch ms: trials %.1f  thermo %.1f  variants %.1f  target pass %.1f  background pass %.1f  multiplex+scatter %.1f\n",
		g_opt_t[0], g_opt_t[1], g_opt_t[2], g_opt_t[3], g_opt_t[4], g_opt_t[5]);
	for(uint32_t i = 0;i < n;++i){
		best_out[i].f = word_of(st[i].best_f); best_out[i].r = word_of(st[i].best_r);
		if(score_out){ score_out[3*i] = st[i].best.tc; score_out[3*i + 1] = st[i].best.bc; score_out[3*i + 2] = st[i].best.ov; }
		if(iterations_out) iterations_out[i] = st[i].iters;
	}
	return PCR_OK;
}

int pcr_optimization_move(pcr_ctx *ctx, const pcr_pair *assay, int move, int side, const pcr_optimize_args *o, const pcr_pair *pool, uint32_t n_pool,
	const float *score_threshold, pcr_word128 *word_out, float *score_out, float *base_score_out)
{
	if(!ctx){ g_err = "pcr_optimization_move: bad argument"; return PCR_ERR_ARG; }
	const bool args_ok = assay && check_opt_args(o) && (side == 0 || side == 1) && move >= 0 && move <= PCR_MOVE_GROW3 && word_out && score_out && !(n_pool && !pool);
	if(!args_ok) g_err = "pcr_optimization_move: bad argument";
	if(ctx->shard_comm){
		int rc0 = args_ok ? enter_device(ctx) : PCR_ERR_ARG;
		uint64_t fp = 0;
		if(rc0 == PCR_OK){
			const uint64_t extra[3] = {(uint64_t)move, (uint64_t)side, score_threshold ? 1ull : 0ull};
			fp = sh_hash(opt_fingerprint(2, assay, 1, o, pool, n_pool), extra, sizeof(extra));
			if(score_threshold) fp = sh_hash(fp, score_threshold, 3*sizeof(float));
		}
		rc0 = shard_agree(ctx, fp, rc0, "pcr_optimization_move");
		if(rc0 != PCR_OK) return rc0;
	}
	if(!args_ok) return PCR_ERR_ARG;
	DRAIN(ctx);
	HIP_TRY(hipSetDevice(ctx->device));
	const bool multiplex = o->use_multiplex != 0;
	PoolPlanes P;
	if(multiplex){ for(uint32_t i = 0;i < n_pool;++i){ P.pp.push_back(pcrhost::planes_of_word(pool[i].f.w)); P.pp.push_back(pcrhost::planes_of_word(pool[i].r.w)); } }
	pcr_optimize_args one = *o;
	one.n_moves = 1; one.moves[0] = move;
	std::vector<IterAssay> A(1);
	A[0].f = pcrhost::planes_of_word(assay->f.w); A[0].r = pcrhost::planes_of_word(assay->r.w);
	const int rc = evaluate_iteration(ctx, A, &one, multiplex ? &P : nullptr, side, move);
	if(rc != PCR_OK) return rc;
	ScoreH thr = A[0].base;
	if(score_threshold){ thr.tc = score_threshold[0]; thr.bc = score_threshold[1]; thr.ov = score_threshold[2]; }
	if(base_score_out){ base_score_out[0] = A[0].base.tc; base_score_out[1] = A[0].base.bc; base_score_out[2] = A[0].base.ov; }
	const float partial = multiplex ? reuse_term(pool_overlap(side ? A[0].f : A[0].r, P)) : 0.0f;
	Planes w; ScoreH sc;
	const std::pair<uint32_t, uint32_t> sp = A[0].span[side][0];
	decide_move(A[0].rows[side].data() + sp.first, sp.second - sp.first, thr, move, multiplex, partial, w, sc);
	*word_out = word_of(w);
	score_out[0] = sc.tc; score_out[1] = sc.bc; score_out[2] = sc.ov;
	return PCR_OK;
}

} // extern "C"

#include "pcr_degenerate.inc"
#include "pcr_shard_design.inc"
#include "pcr_design.inc"
