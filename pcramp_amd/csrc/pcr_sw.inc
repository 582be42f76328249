// Smith-Waterman primer x template alignment (included by pcr_device.hip).
//
// Reference: SO::SeqOverlap::align_smith_waterman, nucleic-acid mode (seq_overlap.cpp:347-609):
// match +2 when the IUPAC sets intersect else -3, gap open -5 / extend -2 (:60-67), three states
// M / I_query / I_target, alignment START coordinates carried with every state (:483-574), and a
// running maximum taken with !(X.M < max) so ties go to the LAST cell in row-major order (:583).
//
// Mapping: one 32-lane half-wavefront per alignment, lane i = query row i (|q| <= 32, the Word
// capacity).  The cell front advances along anti-diagonals: at step t lane i computes column
// j = t - i.  Its left neighbour C is its own previous cell (registers); its upper neighbour B is
// lane i-1's previous cell and its diagonal neighbour A is the B it received one step earlier,
// so each step moves ONE cell (five packed 32-bit words) down the lanes with wave shuffles.  The
// template streams through the same shuffle chain (lane 0 feeds column t), so neither sequence
// is re-read: HBM traffic is |q| + |t| codes + one 16-byte result per alignment.
// The reference evaluates 8 such alignments as int16 SSE lanes; values here are int32 in
// registers but never leave the int16 range (|score| <= 64, coordinates < 2^15).

struct SwOut { int16_t score, q_start, q_stop, t_start, t_stop; uint8_t last1, last2, valid, pad; };

struct SwJob { uint32_t q; uint32_t tlen; uint64_t t_off; };   // q = index into qcodes/qlen; target codes at tcodes + t_off

struct SwCell { int M, Iq, It, Msi, Msj, Iqsi, Iqsj, Itsi, Itsj; };

__device__ __forceinline__ uint32_t pack16(int a, int b) { return ((uint32_t)a & 0xFFFFu) | ((uint32_t)b << 16); }
__device__ __forceinline__ int lo16(uint32_t v) { return (int)(int16_t)(v & 0xFFFFu); }
__device__ __forceinline__ int hi16(uint32_t v) { return (int)(int16_t)(v >> 16); }

constexpr int SW_THREADS = 256;
constexpr int SW_GAP_OPEN = -5, SW_GAP_EXT = -2, SW_MATCH = 2, SW_MISMATCH = -3;

// One alignment on a 32-lane half-wavefront.  tcode(col) = template code of column col (any col < tlen).
// COORDS = false: the score-only form for callers that read nothing but `score` and the last two aligned template bases
// (find_background_match, find_multiplex_background_match: background_match.cpp:82-120,244-267) -- the six start-coordinate
// fields of a cell are neither computed nor shuffled (two shuffles per step instead of five, a third of the selects); the
// maximum cell is chosen exactly as in the full form, so score and t_stop are the same.
template<bool COORDS, class TCode>
__device__ __forceinline__ void sw_lane(bool have_job, int qlen, int tlen, int qi, TCode tcode, SwOut &r)
{
	const int i = threadIdx.x & 31;                 // query row owned by this lane
	// this lane's previous cell; before its first column it is the first-column boundary of row i
	// (curr_row[0], seq_overlap.cpp:404-411): M = 0, gaps = open, M_start = (i+1, 0)
	SwCell C = {0, SW_GAP_OPEN, SW_GAP_OPEN, i + 1, 0, 0, 0, 0, 0};
	SwCell A = {0, SW_GAP_OPEN, SW_GAP_OPEN, 0, 0, 0, 0, 0, 0};   // the B of the previous step
	int tcur = 0;            // template code of this lane's current column
	int chunk = 0;           // lane l holds template code 32*c + l of the current 32-column chunk
	int best = -32768, best_j = 0, best_si = 0, best_sj = 0;

	const int n_steps = (qlen > 0 && tlen > 0) ? (qlen + tlen - 1) : 0;
	// every lane of the wave runs the same number of steps (shuffles need all lanes): take the max of the two jobs
	int steps_wave = n_steps;
	steps_wave = max(steps_wave, __shfl_xor(steps_wave, 32));

	for(int t = 0;t < steps_wave;++t){
		if((t & 31) == 0){
			const int col = t + i;
			chunk = (col < tlen) ? tcode(col) : 0;
		}
		// the cell lane i-1 produced last step, and the template code it used, move down one lane
		const uint32_t s0 = __shfl_up(pack16(C.M, C.Iq), 1, 32);
		const uint32_t s1 = __shfl_up(pack16(C.It, tcur), 1, 32);
		uint32_t s2 = 0, s3 = 0, s4 = 0;
		if constexpr (COORDS){
			s2 = __shfl_up(pack16(C.Msi, C.Msj), 1, 32);
			s3 = __shfl_up(pack16(C.Iqsi, C.Iqsj), 1, 32);
			s4 = __shfl_up(pack16(C.Itsi, C.Itsj), 1, 32);
		}
		const int tfeed = __shfl(chunk, t & 31, 32);   // template code of column t, for lane 0
		SwCell B;
		int tnew;
		if(i == 0){
			// top boundary row (last_row, seq_overlap.cpp:383-392): index j+1 for B, index j for A
			B.M = 0; B.Iq = B.It = SW_GAP_OPEN; B.Msi = 0; B.Msj = t + 1; B.Iqsi = B.Iqsj = B.Itsi = B.Itsj = 0;
			A.M = 0; A.Iq = A.It = SW_GAP_OPEN; A.Msi = 0; A.Msj = t; A.Iqsi = A.Iqsj = A.Itsi = A.Itsj = 0;
			tnew = tfeed;
		}
		else{
			B.M = lo16(s0); B.Iq = hi16(s0); B.It = lo16(s1); tnew = hi16(s1);
			B.Msi = lo16(s2); B.Msj = hi16(s2); B.Iqsi = lo16(s3); B.Iqsj = hi16(s3); B.Itsi = lo16(s4); B.Itsj = hi16(s4);
		}
		const int j = t - i;
		const bool active = (j >= 0) && (j < tlen) && (i < qlen);
		if(active){
			tcur = tnew;
			SwCell X;
			const int tmp_c = max(max(A.M, A.Iq), A.It);                          // :436
			const int s = ((qi & tcur) != 0) ? SW_MATCH : SW_MISMATCH;            // :440-444
			X.M = max(tmp_c, 0) + s;                                              // :455-458
			X.Msi = X.Msj = X.Iqsi = X.Iqsj = X.Itsi = X.Itsj = 0;
			bool m;
			if constexpr (COORDS){
				m = (A.M < A.Iq) || (A.M < A.It);                                 // :483-488
				X.Msi = m ? 0 : A.Msi; X.Msj = m ? 0 : A.Msj;
				m = !(A.Iq < A.It) && (A.Iq > A.M);                               // :491-503
				X.Msi = m ? A.Iqsi : X.Msi; X.Msj = m ? A.Iqsj : X.Msj;
				m = (A.It > A.M) && (A.It > A.Iq);                                // :506-518
				X.Msi = m ? A.Itsi : X.Msi; X.Msj = m ? A.Itsj : X.Msj;
				m = (0 > tmp_c);                                                  // :522-532
				X.Msi = m ? i : X.Msi; X.Msj = m ? j : X.Msj;
			}
			int tb = max(C.M, 0) + SW_GAP_OPEN, tc = max(C.Iq, 0) + SW_GAP_EXT;   // :536-553
			X.Iq = max(tb, tc);
			if constexpr (COORDS){ m = (tb < tc); X.Iqsi = m ? C.Iqsi : C.Msi; X.Iqsj = m ? C.Iqsj : C.Msj; }
			tb = max(B.M, 0) + SW_GAP_OPEN; tc = max(B.It, 0) + SW_GAP_EXT;       // :557-574
			X.It = max(tb, tc);
			if constexpr (COORDS){ m = (tb < tc); X.Itsi = m ? B.Itsi : B.Msi; X.Itsj = m ? B.Itsj : B.Msj; }
			if(!(X.M < best)){ best = X.M; best_j = j; best_si = X.Msi; best_sj = X.Msj; }   // row-local form of :583
			C = X;
		}
		A = B;
	}

	// global maximum; ties -> larger row, then (already) larger column: the last cell in row-major order
	int bi = i;
	if(!(i < qlen) || n_steps == 0) best = -32768;
#pragma unroll
	for(int off = 16;off >= 1;off >>= 1){
		const int ob = __shfl_xor(best, off, 32), oi = __shfl_xor(bi, off, 32), oj = __shfl_xor(best_j, off, 32);
		const int osi = __shfl_xor(best_si, off, 32), osj = __shfl_xor(best_sj, off, 32);
		if(ob > best || (ob == best && oi > bi)){ best = ob; bi = oi; best_j = oj; best_si = osi; best_sj = osj; }
	}
	r.pad = 0;
	if(have_job && i == 0){
		if(best >= 0){   // the reference's running maximum starts at 0 (:399): only cells >= 0 ever take it
			r.score = (int16_t)best; r.valid = 1;
			r.q_start = (int16_t)best_si; r.q_stop = (int16_t)bi; r.t_start = (int16_t)best_sj; r.t_stop = (int16_t)best_j;
			r.last1 = r.last2 = 15;                                               // seq_overlap.h:1266-1286
			if(best_j >= 1 && best_j < tlen){ r.last1 = (uint8_t)tcode(best_j - 1); r.last2 = (uint8_t)tcode(best_j); }
		}
		else{ r.score = 0; r.valid = 0; r.q_start = r.q_stop = r.t_start = r.t_stop = 0; r.last1 = r.last2 = 15; }
	}
}

template<bool COORDS>
__global__ __launch_bounds__(SW_THREADS) void k_sw(const SwJob *__restrict__ jobs, uint32_t n_jobs,
	const uint8_t *__restrict__ qcodes /* [nq][32] */, const uint8_t *__restrict__ qlens,
	const uint8_t *__restrict__ tcodes, SwOut *__restrict__ out)
{
	const uint32_t job = (blockIdx.x*SW_THREADS + threadIdx.x) >> 5;
	const int i = threadIdx.x & 31;
	const bool have_job = job < n_jobs;
	SwJob jb; jb.q = 0; jb.tlen = 0; jb.t_off = 0;
	if(have_job) jb = jobs[job];
	const int qlen = have_job ? (int)qlens[jb.q] : 0;
	const int qi = (have_job && i < qlen) ? (int)qcodes[(size_t)jb.q*32 + i] : 0;
	const uint8_t *tsrc = tcodes + jb.t_off;
	SwOut r;
	sw_lane<COORDS>(have_job, qlen, (int)jb.tlen, qi, [&](int col){ return (int)tsrc[col]; }, r);
	if(have_job && i == 0) out[job] = r;
}

// The same lanes straight from reference Words (pcr_sw_align_words): query word k against template word k.  The code
// strings SeqOverlap::pack_query_slots / pack_target_slots(Word) would build (size() slots starting at start(),
// seq_overlap.h:828-857,1099-1125) are read out of the 16-byte words on the fly -- no conversion pass, no code arrays.
__device__ __forceinline__ int sw_word_nibble(const uint64_t w0, const uint64_t w1, int k)   // slot k of a Word, 0 past slot 31 (word.h: slot k at bits (15 - k%16)*4 of w[k/16])
{
	if(k > 31) return 0;
	const uint64_t w = (k < 16) ? w0 : w1;
	return (int)((w >> ((15 - (k & 15))*4)) & 0xFull);
}

__global__ __launch_bounds__(SW_THREADS) void k_sw_words(const pcr_word128 *__restrict__ queries, const pcr_word128 *__restrict__ templates,
	uint32_t n_jobs, SwOut *__restrict__ out)
{
	const uint32_t job = (blockIdx.x*SW_THREADS + threadIdx.x) >> 5;
	const int i = threadIdx.x & 31;
	const bool have_job = job < n_jobs;
	uint64_t q0 = 0, q1 = 0, t0 = 0, t1 = 0;
	if(have_job){ q0 = queries[job].w[0]; q1 = queries[job].w[1]; t0 = templates[job].w[0]; t1 = templates[job].w[1]; }
	// occupancy of the 32 slots: every lane looks at its own slot, the half-wave votes
	const uint64_t vq = __ballot(sw_word_nibble(q0, q1, i) != 0), vt = __ballot(sw_word_nibble(t0, t1, i) != 0);
	const uint32_t half = (threadIdx.x >> 5) & 1u;
	const uint32_t oq = (uint32_t)(vq >> (32*half)), ot = (uint32_t)(vt >> (32*half));
	const int qlen = __popc(oq), tlen = __popc(ot);
	const int qstart = oq ? (__ffs(oq) - 1) : 32, tstart = ot ? (__ffs(ot) - 1) : 32;
	const int qi = (i < qlen) ? sw_word_nibble(q0, q1, qstart + i) : 0;
	SwOut r;
	sw_lane<true>(have_job, qlen, tlen, qi, [&](int col){ return sw_word_nibble(t0, t1, tstart + col); }, r);
	if(have_job && i == 0) out[job] = r;
}

// DB entry words -> template code strings exactly as SeqOverlap::pack_target_slots(Word) reads
// them (seq_overlap.h:1099-1125): size() consecutive slots starting at start().
__global__ void k_entry_codes(const DevEntry *__restrict__ db, uint32_t n, uint32_t cap, const uint32_t *__restrict__ touched,
	const uint32_t *__restrict__ seg_hi, uint8_t *__restrict__ codes, uint8_t *__restrict__ lens)
{
	const uint32_t t = (blockIdx.x*blockDim.x + threadIdx.x) >> 5;
	const int k = threadIdx.x & 31;
	uint32_t e;
	if(!db_slot(t, n, cap, touched, seg_hi, e)) return;
	const Planes w = db[e].w;
	const uint32_t occ = w.a | w.c | w.g | w.t;
	const int len = __popc(occ);
	const int start = occ ? (__ffs(occ) - 1) : 32;
	uint32_t code = 0;
	if(k < len && start + k < 32) code = nibble_at(w, start + k);
	codes[(size_t)e*32 + k] = (uint8_t)code;
	if(k == 0) lens[e] = (uint8_t)len;
}

// nibble store -> one code byte per base (templates of find_multiplex_background_match).  SEQ_CODE_SLICES workgroups per
// sequence, all in the grid's x extent: the set grows with every accepted assay's amplicons and passes the 65 535 a y extent holds.
constexpr uint32_t SEQ_CODE_SLICES = 8;
__global__ void k_seq_codes(const uint32_t *__restrict__ nib, const uint64_t *__restrict__ blk_off, const uint64_t *__restrict__ len,
	const uint64_t *__restrict__ code_off, uint32_t n_seq, uint8_t *__restrict__ codes)
{
	const uint32_t s = blockIdx.x/SEQ_CODE_SLICES, slice = blockIdx.x % SEQ_CODE_SLICES;
	if(s >= n_seq) return;
	const uint64_t L = len[s];
	for(uint64_t p = (uint64_t)slice*blockDim.x + threadIdx.x;p < L;p += (uint64_t)SEQ_CODE_SLICES*blockDim.x){
		const uint32_t w = nib[blk_off[s]*4 + (p >> 3)];
		codes[code_off[s] + p] = (uint8_t)((w >> ((p & 7)*4)) & 0xF);
	}
}

// ---------------------------------------------------------------- find_background_match
struct AmpRec { uint32_t pair, seq, f_entry, r_entry; };

// Same walk as k_pair, but instead of the identity test every candidate amplicon is emitted
// (PCR::collect_candidates' m_amplicons, pcr_assay.cpp:424-438) for the alignment stage.
__global__ void k_pair_emit(const DevEntry *__restrict__ db, uint32_t n, uint32_t db_cap, const uint32_t *__restrict__ touched, const uint32_t *__restrict__ seg_hi,
	const uint32_t *__restrict__ mask, uint32_t mask_words, const OligoDev *__restrict__ oligos, uint32_t n_pairs,
	const uint4 *__restrict__ planes, const uint64_t *__restrict__ blk_off, const uint64_t *__restrict__ len,
	const uint8_t *__restrict__ active, int32_t amp_min, int32_t amp_max,
	AmpRec *__restrict__ recs, uint32_t cap, uint32_t *__restrict__ counter, uint32_t *__restrict__ status)
{
	const uint32_t t = blockIdx.x*blockDim.x + threadIdx.x;
	uint32_t i;
	if(!db_slot(t, n, db_cap, touched, seg_hi, i)) return;
	const DevEntry ei = db[i];
	if(ei.strand != 1) return;
	if(!active[ei.seq]) return;
	const uint32_t hi = seg_hi[ei.seq];
	const int32_t L = (int32_t)len[ei.seq];
	const uint64_t base = blk_off[ei.seq];
	for(uint32_t j = i + 1;j < hi;++j){
		const DevEntry ej = db[j];
		if(ej.loc - ei.loc > amp_max + 128) break;
		if(ej.strand != 2) continue;
		for(uint32_t w = 0;w < mask_words;++w){
			const uint32_t mi = mask[(size_t)i*mask_words + w], mj = mask[(size_t)j*mask_words + w];
			const uint32_t fr = mi & (mj >> 1) & 0x55555555u;
			const uint32_t rf = (mi >> 1) & mj & 0x55555555u;
			uint32_t any = fr | rf;
			while(any){
				const uint32_t bit = __ffs(any) - 1;
				any &= any - 1;
				const uint32_t pair = (w*32 + bit) >> 1;
				if(pair >= n_pairs) break;
				const OligoDev F = oligos[2*pair], R = oligos[2*pair + 1];
				for(int orient = 0;orient < 2;++orient){
					if(!(((orient == 0) ? fr : rf) >> bit & 1u)) continue;
					const OligoDev &P = (orient == 0) ? F : R;
					const OligoDev &M = (orient == 0) ? R : F;
					if(ei.loc + P.stop >= ej.loc - M.stop) continue;
					int32_t amp_start = ei.loc + P.start;
					const int32_t amp_stop = min(ej.loc - M.start, L - 1);
					int32_t amp_len = amp_stop - amp_start + 1;
					if(amp_len < amp_min || amp_len > amp_max) continue;
					if(amp_start < 0){ amp_len += amp_start; amp_start = 0; }
					if(amp_len < 0 || amp_start + amp_len > L){ atomicOr(status, 1u); continue; }
					if(has_split(planes, base, amp_start, amp_len)) continue;
					const uint32_t k = atomicAdd(counter, 1u);
					if(k < cap){
						AmpRec r; r.pair = pair; r.seq = ei.seq;
						r.f_entry = (orient == 0) ? i : j;      // the key matched by F (pcr_assay.cpp:425-438)
						r.r_entry = (orient == 0) ? j : i;
						recs[k] = r;
					}
				}
			}
		}
	}
}

// The same candidate amplicons with one WAVE per sequence (the default path of pcr_background_match).  k_pair_emit gives every DB
// slot a thread that walks all later entries of its sequence through global memory and appends with one atomic per record, all on
// one counter (427 us at C3's 10 000 backgrounds, a quarter of them the ~25 000 same-address atomics).  Here the wave walks the plus-strand entries of
// its sequence one after the other (wave-uniform) with the lanes over the partner entries, keeps its records in LDS and appends them
// with ONE atomic per flush; per-pair record counts (who needs the reference's amplicon order at all, see k_bg_score) are added
// as the records leave.  counters[0] = records emitted (may exceed rec_cap: the host grows the list and repeats).
// STAGED (every sequence's bucket holds at most BGE_STAGE entries and the batch at most 32 * BGE_MW oligos -- the usual case): the
// wave first brings its sequence's entries into LDS -- position and strand packed into one word, and the match_words masks, which
// it computes itself from the entries' planes (lane = oligo, the entries wave-uniform), so neither k_match nor its mask array in
// global memory is needed -- and pairs out of LDS; walking the sequence through global memory cost a chain of three dependent
// loads per plus-strand entry (212 us at C3).  Otherwise the masks come from k_match's array and the entries from the DB.
// Memory latency is what the kernel waits for (r03 counters: 73 % of its wave cycles parked on s_waitcnt): so the LDS a wave needs is
// kept small enough for 7 workgroups per CU (STAGE = 64, the default bucket size), the oligos' start / stop slots sit in LDS (the
// geometry of a candidate needs nothing else), and the records leave through BGE_SUB sub-lists with a counter each (every wave ends
// with one append: on ONE counter those atomics, ~11 ns apiece, would be most of the kernel); k_bg_compact joins the sub-lists.
constexpr int BGE_WAVES = 4, BGE_LIST = 64, BGE_MW = 8, BGE_SUB = 16;
template<int STAGE>
__global__ __launch_bounds__(64*BGE_WAVES) void k_bg_emit(const DevEntry *__restrict__ db, uint32_t n_touched, uint32_t db_cap, const uint32_t *__restrict__ touched,
	const uint32_t *__restrict__ seg_hi, const uint32_t *__restrict__ mask, uint32_t mask_words, const OligoDev *__restrict__ oligos, uint32_t n_pairs,
	const uint4 *__restrict__ planes, const uint64_t *__restrict__ blk_off, const uint64_t *__restrict__ len,
	const uint8_t *__restrict__ active, const uint8_t *__restrict__ has_eos, int32_t amp_min, int32_t amp_max,
	AmpRec *__restrict__ recs, uint32_t sub_cap /* records per sub-list */, uint32_t *__restrict__ sub_count /* [BGE_SUB] */, uint32_t *__restrict__ status)
{
	constexpr bool STAGED = STAGE > 0;
	extern __shared__ uint32_t bge_geom[];                                                 // per oligo: start | stop << 8 (Word::start() / stop())
	__shared__ AmpRec list_all[BGE_WAVES][BGE_LIST + 64];
	__shared__ uint32_t fill_all[BGE_WAVES], base_all[BGE_WAVES];
	__shared__ uint32_t ls_all[STAGED ? BGE_WAVES : 1][STAGED ? STAGE : 1];                 // (loc + LOC_BIAS) | minus strand << 31
	__shared__ uint32_t sm_all[STAGED ? BGE_WAVES : 1][STAGED ? STAGE*BGE_MW : 1];          // masks, entry-major
	__shared__ uint4 sw_all[STAGED ? BGE_WAVES : 1][STAGED ? STAGE : 1];                    // the entries' planes
	for(uint32_t o = threadIdx.x;o < 2*n_pairs;o += blockDim.x) bge_geom[o] = ((uint32_t)oligos[o].start & 0xFFu) | (((uint32_t)oligos[o].stop & 0xFFu) << 8);
	__syncthreads();
	AmpRec *const my_recs = recs + (size_t)(blockIdx.x % BGE_SUB)*sub_cap;
	uint32_t *const my_count = sub_count + (blockIdx.x % BGE_SUB);
	const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
	AmpRec *const list = list_all[wave];
	uint32_t &fill = fill_all[wave];
	uint32_t *const ls = ls_all[STAGED ? wave : 0], *const sm = sm_all[STAGED ? wave : 0];
	if(lane == 0) fill = 0;
	wave_sync();
	auto flush = [&](){
		const uint32_t n = *(volatile uint32_t *)&fill;
		if(n == 0) return;
		if(lane == 0) base_all[wave] = atomicAdd(my_count, n);
		wave_sync();
		const uint32_t base = *(volatile uint32_t *)&base_all[wave];
		for(uint32_t k = lane;k < n;k += 64){
			const AmpRec r = list[k];
			if(base + k < sub_cap) my_recs[base + k] = r;
		}
		wave_sync();
		if(lane == 0) fill = 0;
		wave_sync();
	};
	const uint32_t n_oligo = 2*n_pairs;
	uint4 *const sw = sw_all[STAGED ? wave : 0];
	// this lane's oligos (lane + 64 p) for the mask computation; an oligo past the batch matches nothing (floor 255)
	Planes oq[BGE_MW/2]; uint32_t ofl[BGE_MW/2];
#pragma unroll
	for(int p = 0;p < BGE_MW/2;++p){
		const uint32_t o = (uint32_t)p*64u + lane;
		oq[p].a = oq[p].c = oq[p].g = oq[p].t = 0; ofl[p] = 255u;
		if(STAGED && o < n_oligo){ oq[p] = oligos[o].m; ofl[p] = oligos[o].floor2; }
	}
	for(uint32_t t_idx = blockIdx.x*BGE_WAVES + wave;t_idx < n_touched;t_idx += gridDim.x*BGE_WAVES){
		const uint32_t seq = touched[t_idx];
		if(!active[seq]) continue;
		const uint32_t lo = seq*db_cap, n = seg_hi[seq] - lo;
		const int32_t L = (int32_t)len[seq];
		const uint64_t base = blk_off[seq];
		const bool eos = has_eos[seq] != 0;
		if constexpr (STAGED){
			// entries -> LDS (planes, position | strand), then the masks with lane = oligo and the entries wave-uniform: 64 oligos
			// against one entry per step, the results leave as one ballot = two mask words (an oligo loop per lane = entry waited
			// for a scalar load of the oligo in every iteration: 8 us per sequence)
			for(uint32_t k = lane;k < n;k += 64){
				const DevEntry e = db[lo + k];
				sw[k] = make_uint4(e.w.a, e.w.c, e.w.g, e.w.t);
				ls[k] = ((uint32_t)(e.loc + LOC_BIAS) & 0x7FFFFFFFu) | ((e.strand == 2u) ? 0x80000000u : 0u);
			}
			wave_sync();
#pragma unroll
			for(int p = 0;p < BGE_MW/2;++p){
				if((uint32_t)p*64u >= n_oligo) break;
				for(uint32_t k = 0;k < n;++k){
					const uint4 w = sw[k];                                             // (broadcast read)
					const bool ok = (uint32_t)__popc((w.x & oq[p].a) | (w.y & oq[p].c) | (w.z & oq[p].g) | (w.w & oq[p].t)) >= ofl[p];   // optimize.cpp:291-301
					const uint64_t bal = __ballot(ok);
					if(lane == 0){
						sm[k*mask_words + 2*p] = (uint32_t)bal;
						if(2u*p + 1u < mask_words) sm[k*mask_words + 2*p + 1] = (uint32_t)(bal >> 32);
					}
				}
			}
			wave_sync();
		}
		auto loc_strand = [&](uint32_t k) -> uint32_t {
			if constexpr (STAGED) return ls[k];
			else{ const DevEntry &e = db[lo + k]; return ((uint32_t)(e.loc + LOC_BIAS) & 0x7FFFFFFFu) | ((e.strand == 2u) ? 0x80000000u : 0u); }
		};
		auto mask_of = [&](uint32_t k, uint32_t w) -> uint32_t {
			if constexpr (STAGED) return sm[k*mask_words + w];
			else return mask[(size_t)(lo + k)*mask_words + w];
		};
		for(uint32_t i = 0;i + 1 < n;++i){
			const uint32_t ils = loc_strand(i);                                    // (wave-uniform)
			if(ils >> 31) continue;                                                // a plus-strand site leads (pcr_assay.cpp:349)
			const int32_t iloc = (int32_t)(ils & 0x7FFFFFFFu) - LOC_BIAS;
			for(uint32_t j0 = i + 1;j0 < n;j0 += 64){
				const uint32_t j = j0 + lane;
				const uint32_t jls = (j < n) ? loc_strand(j) : 0x7FFFFFFFu;
				const int32_t jloc = (int32_t)(jls & 0x7FFFFFFFu) - LOC_BIAS;
				const bool near = (j < n) && (jloc - iloc <= amp_max + 128);       // entries are sorted by loc: once a chunk holds no near entry, none follows
				if(near && (jls >> 31)){
					for(uint32_t w = 0;w < mask_words;++w){
						const uint32_t mi = mask_of(i, w), mj = mask_of(j, w);
						const uint32_t fr = mi & (mj >> 1) & 0x55555555u;
						const uint32_t rf = (mi >> 1) & mj & 0x55555555u;
						uint32_t any = fr | rf;
						while(any){
							const uint32_t bit = __ffs(any) - 1;
							any &= any - 1;
							const uint32_t pair = (w*32 + bit) >> 1;
							if(pair >= n_pairs) break;
							const uint32_t gf = bge_geom[2*pair], gr = bge_geom[2*pair + 1];
							for(int orient = 0;orient < 2;++orient){
								if(!(((orient == 0) ? fr : rf) >> bit & 1u)) continue;
								const uint32_t gp = (orient == 0) ? gf : gr, gm = (orient == 0) ? gr : gf;
								const int32_t p_start = (int32_t)(int8_t)(gp & 0xFFu), p_stop = (int32_t)(int8_t)(gp >> 8);
								const int32_t m_start = (int32_t)(int8_t)(gm & 0xFFu), m_stop = (int32_t)(int8_t)(gm >> 8);
								if(iloc + p_stop >= jloc - m_stop) continue;                   // pcr_assay.cpp:367-370
								int32_t amp_start = iloc + p_start;
								const int32_t amp_stop = min(jloc - m_start, L - 1);
								int32_t amp_len = amp_stop - amp_start + 1;
								if(amp_len < amp_min || amp_len > amp_max) continue;
								if(amp_start < 0){ amp_len += amp_start; amp_start = 0; }
								if(amp_len < 0 || amp_start + amp_len > L){ atomicOr(status, 1u); continue; }   // sequence.cpp:306 throw
								if(eos && has_split(planes, base, amp_start, amp_len)) continue;
								AmpRec r; r.pair = pair; r.seq = seq;
								r.f_entry = (orient == 0) ? lo + i : lo + j;               // the key matched by F (pcr_assay.cpp:425-438)
								r.r_entry = (orient == 0) ? lo + j : lo + i;
								const uint32_t slot = atomicAdd(&fill, 1u);
								if(slot < BGE_LIST + 64) list[slot] = r;
								else{                                                      // (more than 64 records from one lane's partner: straight to the sub-list)
									const uint32_t k = atomicAdd(my_count, 1u);
									if(k < sub_cap) my_recs[k] = r;
								}
							}
						}
					}
				}
				wave_sync();
				if(*(volatile uint32_t *)&fill > BGE_LIST + 64){ if(lane == 0) fill = BGE_LIST + 64; wave_sync(); }   // the overflowing records went out on their own
				if(*(volatile uint32_t *)&fill >= BGE_LIST) flush();
				if(!__ballot(near)) break;
			}
		}
		if constexpr (STAGED) wave_sync();                                         // the staged entries are replaced by the wave's next sequence
	}
	flush();
}

// k_bg_emit's sub-lists -> one list, and the number of records per pair (who needs the reference's amplicon order, k_bg_score):
// counted per workgroup in LDS and added to pair_count[] once per workgroup and pair -- a global atomic per RECORD lands ~25 000
// of them on the two or three cache lines that hold the counters, and atomics on one line run one after the other (~11 ns each: that
// was 140 of k_bg_emit's 157 us).  counters[0] = records in the list, counters[3] = records emitted (more, when a sub-list
// overflowed: counters[2] bit 0; the host grows the lists and repeats the call).  Launched with few, large workgroups.
constexpr uint32_t BGC_LDS_PAIRS = 8192;
__global__ __launch_bounds__(1024) void k_bg_compact(const AmpRec *__restrict__ sub_recs, uint32_t sub_cap, const uint32_t *__restrict__ sub_count, AmpRec *__restrict__ recs,
	uint32_t *__restrict__ counters, uint32_t *__restrict__ pair_count, uint32_t n_pairs)
{
	__shared__ uint32_t hist[BGC_LDS_PAIRS];
	const bool lds_hist = n_pairs <= BGC_LDS_PAIRS;
	if(lds_hist){ for(uint32_t p = threadIdx.x;p < n_pairs;p += blockDim.x) hist[p] = 0; }
	__syncthreads();
	uint32_t start[BGE_SUB + 1];
	uint32_t run = 0, over = 0, true_total = 0;
	for(int q = 0;q < BGE_SUB;++q){ start[q] = run; run += min(sub_count[q], sub_cap); true_total += sub_count[q]; over |= (sub_count[q] > sub_cap) ? 1u : 0u; }
	start[BGE_SUB] = run;
	if(blockIdx.x == 0 && threadIdx.x == 0){ counters[0] = run; counters[2] = over; counters[3] = true_total; }
	for(uint32_t k = blockIdx.x*blockDim.x + threadIdx.x;k < run;k += gridDim.x*blockDim.x){
		int q = 0;
		while(k >= start[q + 1]) ++q;
		const AmpRec r = sub_recs[(size_t)q*sub_cap + (k - start[q])];
		recs[k] = r;
		if(lds_hist) atomicAdd(&hist[r.pair], 1u); else atomicAdd(&pair_count[r.pair], 1u);
	}
	__syncthreads();
	if(lds_hist){ for(uint32_t p = threadIdx.x;p < n_pairs;p += blockDim.x){ if(hist[p]) atomicAdd(&pair_count[p], hist[p]); } }
}

// Score-only Smith-Waterman of the candidate amplicons' four lanes straight from the records (no job list, no code strings):
// job 4a + l of amplicon a: query 4*pair + l (F, (F), R, (R)) against the key word of the F-site (l < 2) or the R-site entry,
// whose codes are read out of the DB entry's planes as SeqOverlap::pack_target_slots(Word) would spell them (seq_overlap.h:1099-1125).
// Persistent grid; the record count is on the device (k_bg_emit's counter, clamped to the list's capacity).
// lane l receives lane l - 1's value (lane 0: 0): a DPP move across the whole wave, no LDS crossbar (ds_bpermute)
__device__ __forceinline__ uint32_t wave_shr1(uint32_t v) { return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x138, 0xf, 0xf, false); }   // wave_shr:1

// The score-only alignment of a query against a 32-slot key WORD held in registers (both halves of the wave their own job),
// COLUMN-parallel: lane j = template column j, the rows one after the other -- |q| steps instead of the |q| + |t| - 1 of the
// anti-diagonal sweep, in which a 22 x 32 matrix keeps 41 % of the lane-steps busy.  What makes a whole row computable at once:
//   * downstream of a cell only max(M, 0), max(Iq, 0) and max(It, 0) are ever used (seq_overlap.cpp:436-458,536-574: every use is
//     under a max with 0), M itself only by the running maximum; so a cell is (M, Uq, Ut) with U = max(I, 0);
//   * M[i][j] = max(max(M,0), Uq, Ut)[i-1][j-1] + s: one max3 in the lane that owns the cell above-left, one DPP shift;
//   * Ut[i][j] = max(0, max(M[i-1][j],0) - 5, Ut[i-1][j] - 2): the lane's own previous row;
//   * Uq[i][j] = max(0, max over k < j of (max(M[i][k],0) - 5 - 2 (j-1-k))): the horizontal gap chain of the row unrolled -- a
//     prefix maximum with a decay of 2 per column: an exclusive shift and five DPP steps (row_shr 1, 2, 4, 8, row_bcast:15).
// The maximum cell is the reference's: the last one in row-major order among the cells holding the largest M (:583) -- a lane
// keeps the LAST row of its column's maximum, the reduction prefers the larger row, then the larger column.  No LDS traffic.
// (The r03 counters of the first version -- anti-diagonal, three ds_bpermute per step and a wait behind each: 1.1e7 LDS-crossbar
// instructions per launch, 44 % of the wave cycles stalled at issue.)
template<int CTRL, int ROW_MASK> __device__ __forceinline__ int sw_dpp(int old, int v) { return __builtin_amdgcn_update_dpp(old, v, CTRL, ROW_MASK, 0xf, false); }

__device__ __forceinline__ void sw_word_score(bool have_job, int qlen, int qi /* this lane's ROW code: query base lane & 31 */, const Planes w, SwOut &r)
{
	constexpr int NEG = -4096;
	const int j = threadIdx.x & 31, half = (threadIdx.x >> 5) & 1;
	const bool col0 = j == 0;
	const uint32_t occ = w.a | w.c | w.g | w.t;
	const int tlen = __popc(occ), tstart = occ ? (__ffs(occ) - 1) : 32;
	// rows of the query by base: bit i of qa = query base i may be A, ... (the lanes hold the query one base each)
	const uint32_t qa = (uint32_t)(__ballot(qi & 1) >> (32*half)), qc = (uint32_t)(__ballot(qi & 2) >> (32*half));
	const uint32_t qg = (uint32_t)(__ballot(qi & 4) >> (32*half)), qt = (uint32_t)(__ballot(qi & 8) >> (32*half));
	// this lane's template column (slot tstart + j; past the word or the template: nothing) and the rows that match it (seq_overlap.cpp:440-444)
	const uint32_t tc = (j < tlen && tstart + j < 32) ? nibble_at(w, tstart + j) : 0u;
	const uint32_t colmask = ((tc & 1u) ? qa : 0u) | ((tc & 2u) ? qc : 0u) | ((tc & 4u) ? qg : 0u) | ((tc & 8u) ? qt : 0u);
	int pM = 0, pUq = 0, pUt = 0, pV = SW_GAP_OPEN;            // the row above: the top boundary (:383-392) -- M = 0, gaps closed; V = max(M, 0) + open
	int best = -32768, best_i = 0;
	const int rows = (tlen > 0) ? qlen : 0;
	const int rows_wave = max(rows, __shfl_xor(rows, 32));   // (DPP moves need every lane: both halves run the longer query's rows)
	for(int i = 0;i < rows_wave;++i){
		int tmp0 = sw_dpp<0x138, 0xf>(0, max(max(pM, pUq), pUt));                // the cell above-left (wave_shr:1); >= 0 already, :436,455
		if(col0) tmp0 = 0;                                                       // first-column boundary (:404-411): M = 0, gaps closed
		const int M = tmp0 + (((colmask >> i) & 1u) ? SW_MATCH : SW_MISMATCH);
		const int Ut = max(max(pV, pUt + SW_GAP_EXT), 0);                        // :557-574
		const int V = max(M, 0) + SW_GAP_OPEN;
		int e = sw_dpp<0x138, 0xf>(NEG, V);                                      // the gap opened from the cell to the left ...
		if(col0) e = NEG;
		e = max(e, sw_dpp<0x111, 0xf>(NEG, e + 1*SW_GAP_EXT));                   // ... or extended from further left: row_shr:1, 2, 4, 8,
		e = max(e, sw_dpp<0x112, 0xf>(NEG, e + 2*SW_GAP_EXT));
		e = max(e, sw_dpp<0x114, 0xf>(NEG, e + 4*SW_GAP_EXT));
		e = max(e, sw_dpp<0x118, 0xf>(NEG, e + 8*SW_GAP_EXT));
		e = max(e, sw_dpp<0x142, 0xa>(NEG, e) + ((j & 15) + 1)*SW_GAP_EXT);      // then over the 16-lane row boundary (row_bcast:15 into rows 1, 3)
		const int Uq = max(e, 0);                                                // :536-553
		if(j < tlen && i < rows && !(M < best)){ best = M; best_i = i; }         // column-local form of :583
		pM = M; pUq = Uq; pUt = Ut; pV = V;
	}
	// global maximum; ties -> larger row, then larger column: the last cell in row-major order
	int bj = j;
	if(!(j < tlen) || rows == 0) best = -32768;
#pragma unroll
	for(int off = 16;off >= 1;off >>= 1){
		const int ob = __shfl_xor(best, off, 32), oi = __shfl_xor(best_i, off, 32), oj = __shfl_xor(bj, off, 32);
		if(ob > best || (ob == best && (oi > best_i || (oi == best_i && oj > bj)))){ best = ob; best_i = oi; bj = oj; }
	}
	r.pad = 0; r.q_start = r.t_start = 0;
	if(have_job && j == 0){
		if(best >= 0){   // the reference's running maximum starts at 0 (:399): only cells >= 0 ever take it
			r.score = (int16_t)best; r.valid = 1; r.q_stop = (int16_t)best_i; r.t_stop = (int16_t)bj;
			r.last1 = r.last2 = 15;                                               // seq_overlap.h:1266-1286
			if(bj >= 1 && bj < tlen){
				r.last1 = (tstart + bj - 1 < 32) ? (uint8_t)nibble_at(w, tstart + bj - 1) : 0;
				r.last2 = (tstart + bj < 32) ? (uint8_t)nibble_at(w, tstart + bj) : 0;
			}
		}
		else{ r.score = 0; r.valid = 0; r.q_stop = r.t_stop = 0; r.last1 = r.last2 = 15; }
	}
}

__global__ __launch_bounds__(SW_THREADS) void k_sw_bg(const AmpRec *__restrict__ recs, const uint32_t *__restrict__ counters, uint32_t rec_cap,
	const DevEntry *__restrict__ db, const uint8_t *__restrict__ qcodes, const uint8_t *__restrict__ qlens, SwOut *__restrict__ out)
{
	const uint32_t n_jobs = 4u*min(counters[0], rec_cap);
	const int i = threadIdx.x & 31;
	const uint32_t hw = (blockIdx.x*SW_THREADS + threadIdx.x) >> 5, n_hw = (gridDim.x*SW_THREADS) >> 5;
	// both halves of a wave must run the same number of rounds (the lanes shuffle): rounds are counted per wave
	for(uint32_t job0 = (hw & ~1u);job0 < n_jobs;job0 += n_hw){
		const uint32_t job = job0 + (hw & 1u);
		const bool have_job = job < n_jobs;
		AmpRec a; a.pair = a.seq = a.f_entry = a.r_entry = 0;
		if(have_job) a = recs[job >> 2];
		const uint32_t l = job & 3u, q = 4u*a.pair + l;
		Planes w; w.a = w.c = w.g = w.t = 0;
		if(have_job) w = db[(l < 2u) ? a.f_entry : a.r_entry].w;
		const int qlen = have_job ? (int)qlens[q] : 0;
		const int qi = (have_job && i < qlen) ? (int)qcodes[(size_t)q*32 + i] : 0;
		SwOut r;
		sw_word_score(have_job, qlen, qi, w, r);
		if(have_job && i == 0) out[job] = r;
	}
}

// ---- the reference's amplicon ORDER (reference-identical mode of pcr_background_match)
// PCR::find_background_match walks background_amplicons two at a time and drops the second of a couple once its
// index reaches the number of SEQUENCES (`(i + 1) >= num_seq`, background_match.cpp:122).  Which amplicons that
// hits depends on their order in the deque: {F(+),R(-)} before {R(+),F(-)} (pcr_assay.cpp:39-58), inside an
// orientation by sequence, plus site, minus site (the sorted sweep of find_amplicon_match, pcr_assay.cpp:338-441).
// k_pair_emit appends in whatever order the lanes get there, so the records are sorted by that key (and then,
// stably, by pair) and every record learns its index inside its pair's list.
__global__ void k_amp_keys(const AmpRec *__restrict__ recs, uint32_t n, uint32_t db_cap, uint64_t *__restrict__ keys, uint32_t *__restrict__ index)
{
	const uint32_t k = blockIdx.x*blockDim.x + threadIdx.x;
	if(k >= n) return;
	index[k] = k;                                          // the sorts move record indices, not the 32-byte records
	const AmpRec r = recs[k];
	const uint32_t plus = min(r.f_entry, r.r_entry), minus = max(r.f_entry, r.r_entry);   // the plus-strand site is the earlier DB slot
	const uint64_t orient = (r.f_entry > r.r_entry) ? 1u : 0u;                             // 1: R on the plus strand
	const uint32_t base = r.seq*db_cap;
	keys[k] = (orient << 58) | ((uint64_t)r.seq << 34) | ((uint64_t)(plus - base) << 17) | (uint64_t)(minus - base);
}

__global__ void k_amp_pair_keys(const AmpRec *__restrict__ recs, const uint32_t *__restrict__ index, uint32_t n, uint32_t *__restrict__ keys)
{
	const uint32_t k = blockIdx.x*blockDim.x + threadIdx.x;
	if(k < n) keys[k] = recs[index[k]].pair;
}

__global__ void k_amp_gather(const AmpRec *__restrict__ recs, const uint32_t *__restrict__ index, uint32_t n, AmpRec *__restrict__ out)
{
	const uint32_t k = blockIdx.x*blockDim.x + threadIdx.x;
	if(k < n) out[k] = recs[index[k]];
}

// recs sorted by pair: first index of every pair's run
__global__ void k_amp_pair_start(const AmpRec *__restrict__ recs, uint32_t n, uint32_t *__restrict__ pair_start)
{
	const uint32_t k = blockIdx.x*blockDim.x + threadIdx.x;
	if(k >= n) return;
	if(k == 0 || recs[k - 1].pair != recs[k].pair) pair_start[recs[k].pair] = k;
}

// four alignment jobs per amplicon, in the reference's lane order (background_match.cpp:46-62):
// 0: F + f key, 1: (F) + f key, 2: R + r key, 3: (R) + r key.   Query index = 4*pair + lane.
__global__ void k_bg_jobs(const AmpRec *__restrict__ recs, uint32_t n, const uint8_t *__restrict__ entry_lens, SwJob *__restrict__ jobs)
{
	const uint32_t k = blockIdx.x*blockDim.x + threadIdx.x;
	if(k >= 4*n) return;
	const AmpRec r = recs[k >> 2];
	const uint32_t lane = k & 3;
	const uint32_t e = (lane < 2) ? r.f_entry : r.r_entry;
	SwJob j; j.q = 4*r.pair + lane; j.tlen = entry_lens[e]; j.t_off = (uint64_t)e*32;
	jobs[k] = j;
}

struct BgPairDev { float f_norm, r_norm; uint8_t fp1, fp2, fm1, fm2, rp1, rp2, rm1, rm2; };

__device__ __forceinline__ float taq_corr(uint32_t p1, uint32_t p2, uint32_t t1, uint32_t t2)   // word.cpp:249-294
{
	if(!nondegen(p1) || !nondegen(p2) || !nondegen(t1) || !nondegen(t2)) return 1.0f;
	return fminf(1.0f, c_taq_mama[16*(4*taq_idx(t2) + taq_idx(t1)) + (4*taq_idx(p2) + taq_idx(p1))]);
}

// background_match.cpp:82-120 for one amplicon: normalised score products, TaqMAMA, sqrt, threshold.
// pair_start != nullptr: recs are in the reference's order and the odd-indexed amplicon of a couple is dropped once
// its index reaches n_seq (background_match.cpp:122); nullptr: every amplicon counts.
// n_dev != nullptr: the record count is on the device (grid-stride over min(*n_dev, n)).  pair_count != nullptr (records in NO
// particular order): a pair with more candidate amplicons than there are sequences would lose some of them to that rule, and which
// ones depends on the reference's order -- the kernel raises bit 1 of order_flag and the host repeats the call on the ordered path;
// as long as no pair has more, the rule drops nothing and the order does not matter.
__global__ void k_bg_score(const AmpRec *__restrict__ recs, uint32_t n, const uint32_t *__restrict__ n_dev, const SwOut *__restrict__ sw, const BgPairDev *__restrict__ bp,
	float threshold, int use_taq, uint64_t *__restrict__ bits, uint64_t bit_words, const uint32_t *__restrict__ pair_start, uint32_t n_seq,
	const uint32_t *__restrict__ pair_count, uint32_t *__restrict__ order_flag)
{
	if(n_dev) n = min(*n_dev, n);
	for(uint32_t k = blockIdx.x*blockDim.x + threadIdx.x;k < n;k += gridDim.x*blockDim.x){
	const AmpRec r = recs[k];
	if(pair_start){
		const uint32_t idx = k - pair_start[r.pair];
		if((idx & 1u) && idx >= n_seq) continue;
	}
	if(pair_count && pair_count[r.pair] > n_seq){ atomicOr(order_flag, 2u); continue; }
	const BgPairDev p = bp[r.pair];
	const SwOut l0 = sw[4*k], l1 = sw[4*k + 1], l2 = sw[4*k + 2], l3 = sw[4*k + 3];
	float FpRm = __fmul_rn(__fmul_rn((float)((int)l0.score*(int)l3.score), p.f_norm), p.r_norm);
	float RpFm = __fmul_rn(__fmul_rn((float)((int)l1.score*(int)l2.score), p.f_norm), p.r_norm);
	if(use_taq){
		FpRm = __fmul_rn(FpRm, __fmul_rn(taq_corr(p.fp1, p.fp2, l0.last1, l0.last2), taq_corr(p.rm1, p.rm2, l3.last1, l3.last2)));
		RpFm = __fmul_rn(RpFm, __fmul_rn(taq_corr(p.rp1, p.rp2, l2.last1, l2.last2), taq_corr(p.fm1, p.fm2, l1.last1, l1.last2)));
	}
	const float score = (float)__dsqrt_rn((double)((FpRm > RpFm) ? FpRm : RpFm));   // :100-113
	if(score >= threshold) atomicOr((unsigned long long *)&bits[(size_t)r.pair*bit_words + (r.seq >> 6)], 1ull << (r.seq & 63));
	}
}

// ---------------------------------------------------------------- find_multiplex_background_match
// jobs: for pair p, sequence s, lane l in {F,(F),R,(R)}: index ((p*n_seq + s)*4 + l)
__global__ void k_mx_jobs(uint32_t n_pairs, uint32_t n_seq, const uint64_t *__restrict__ len, const uint64_t *__restrict__ code_off,
	SwJob *__restrict__ jobs)
{
	const uint64_t k = (uint64_t)blockIdx.x*blockDim.x + threadIdx.x;
	if(k >= (uint64_t)n_pairs*n_seq*4) return;
	const uint32_t lane = k & 3;
	const uint64_t ps = k >> 2;
	const uint32_t s = (uint32_t)(ps % n_seq), p = (uint32_t)(ps/n_seq);
	SwJob j; j.q = 4*p + lane; j.tlen = (uint32_t)len[s]; j.t_off = code_off[s];
	jobs[k] = j;
}

// background_match.cpp:244-267: any of the four normalised (TaqMAMA-corrected) scores >= threshold.
__global__ void k_mx_score(uint32_t n_pairs, uint32_t n_seq, const SwOut *__restrict__ sw, const BgPairDev *__restrict__ bp,
	float threshold, int use_taq, uint64_t *__restrict__ bits, uint64_t bit_words)
{
	const uint64_t ps = (uint64_t)blockIdx.x*blockDim.x + threadIdx.x;
	if(ps >= (uint64_t)n_pairs*n_seq) return;
	const uint32_t s = (uint32_t)(ps % n_seq), p = (uint32_t)(ps/n_seq);
	const BgPairDev b = bp[p];
	const uint8_t pl[4][2] = {{b.fp1, b.fp2}, {b.fm1, b.fm2}, {b.rp1, b.rp2}, {b.rm1, b.rm2}};
	bool hit = false;
	for(int l = 0;l < 4;++l){
		const SwOut r = sw[ps*4 + l];
		float sc = __fmul_rn((float)r.score, (l < 2) ? b.f_norm : b.r_norm);
		if(use_taq) sc = __fmul_rn(sc, taq_corr(pl[l][0], pl[l][1], r.last1, r.last2));
		hit |= (sc >= threshold);
	}
	if(hit) atomicOr((unsigned long long *)&bits[(size_t)p*bit_words + (s >> 6)], 1ull << (s & 63));
}
