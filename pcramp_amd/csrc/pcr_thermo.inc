// Nearest-neighbour thermodynamics on the device (included by pcr_device.hip).
//
// What it replaces: NucCruc (nuc_cruc.{h,cpp}; SANTA_LUCIA, non-Dinkelbach, dangles on, <= 17
// paths per maximum cell -- the only configuration pcramp drives, optimize.cpp:49-52,
// main.cpp:533-535) and the three filters built on it: PCR::is_valid (valid_pcr.cpp:5),
// PCR::max_dimer_tm (pcr_assay.cpp:232), PCR::multiplex_compatible (pcr_assay.cpp:815).
//
// Mapping: one lane = one (non-degenerate) oligo or oligo pair; IUPAC expansion happens on the
// host, so a batch of optimiser-move variants becomes thousands of independent lanes.  Every
// lane runs the integer-scaled dG dynamic programme (<= 32 x 32 cells, three states + 3-bit
// trace sets), walks the tied-path enumeration with an explicit branch stack, and evaluates each
// candidate alignment with the SantaLucia stack / loop / bulge / dangle rules in float32.  The DP
// matrix of a lane lives in a global scratch slab laid out cell-major across the 64 lanes of its
// wave (lanes fill the same cell index in lock step -> coalesced), the 49 x 49 dG table and the
// enthalpy / entropy tables sit in LDS / constant memory.
// Float discipline for 1e-6 parity: -ffp-contract=off, correctly rounded divide, and every log()
// (salt, strand concentration) is taken on the host with the same libm the reference uses.

#include "pcr_thermo_tables.inc"

namespace thermo {

enum { bA = 0, bC, bG, bT, bI, bE, bGAP, NB = 7 };
enum { pAT = 3, pTA = 21, pCG = 9, pGC = 15, pGT = 17, pTG = 23, p__ = 48 };
enum { T_DIAG = 1, T_UP = 2, T_LEFT = 4, T_INVALID = 8 };
enum { HOMO_DIMER = 0, HETERO_DIMER = 1, HAIRPIN = 2 };

constexpr int MAXL = 32;                 // Word capacity (options.cpp:854: primers <= 32 nt)
constexpr int STRIDE = MAXL + 1;
constexpr int NCELL = STRIDE*STRIDE;
constexpr int ALN = 4*MAXL + 16;
constexpr int WAVE = 64;
constexpr float ZERO_C = 273.15f, TARGET_T = 273.15f + 37.0f, GAS_R = 1.9872e-3f;   // nuc_cruc.h:103-105
constexpr unsigned MAX_PATH_ENUM = 16;                                              // nuc_cruc.cpp:130

__constant__ float c_H[49*49], c_S[49*49];
__constant__ float c_loop_S[129], c_bulge_S[129], c_hairpin_S[129], c_special_H[131], c_special_S[131];
__constant__ unsigned int c_special_key[131];
__constant__ unsigned char c_wc[49];

__device__ __forceinline__ int PAIR(int q, int t) { return q*NB + t; }

struct Align {
	bool valid;
	float dH, dS, tm;
	unsigned char qa[ALN], ta[ALN];
	int head, tail;
	int first_q, first_t, last_q, last_t;
	__device__ void reset() { valid = false; dH = dS = tm = 0.0f; head = tail = 2*MAXL + 8; first_q = first_t = last_q = last_t = 0; }
	__device__ int size() const { return tail - head; }
};

// a branch point of the trace-back: id = cell*3 + matrix (< 3*33*33 = 3 267: 12 bits), cur = the T_* direction taken (1, 2, 4)
struct Branch { unsigned short id : 12, cur : 4; };
static_assert(sizeof(Branch) == 2, "two bytes per branch point (LDS)");

// The DP matrices as the trace-back needs them.  Of the three score planes only M is read again after the fill (the maximum cells,
// `m < 0`, `m == 0`: nuc_cruc.cpp:1262-1471); of Iq and It the trace-back only asks whether a cell is negative, and the fill itself
// carries them in registers.  So M is an int plane and everything else shares one 16-bit plane: the three 4-bit trace masks, and
// bits 12 / 13 = Iq < 0 / It < 0.  (r02 stored all three planes: 13 KB of LDS per wave instead of 4.3.)
template<int LS> struct Matrix {
	int *M; unsigned short *tr;
	__device__ __forceinline__ int getM(int c) const { return M[c*LS]; }
	__device__ __forceinline__ unsigned trace(int c, int which) const { return (tr[c*LS] >> (4*which)) & 0xF; }
	__device__ __forceinline__ bool negIq(int c) const { return (tr[c*LS] >> 12) & 1u; }
	__device__ __forceinline__ bool negIt(int c) const { return (tr[c*LS] >> 13) & 1u; }
};

template<int LS> struct Engine {
	const int *dg;            // [49][49] in LDS
	float log_na, log_strand;
	unsigned char *q, *t;     // MAXL + 1 codes each (private arrays in the throughput kernel, LDS in the low-latency one)
	int qlen, tlen;
	Matrix<LS> mx;

	__device__ __forceinline__ int step(int prev, int cost) const { return (0 < prev) ? prev - cost : -cost; }

	__device__ __forceinline__ static void pack_codes(const unsigned char *Tq, unsigned long long &tp0, unsigned long long &tp1)
	{
		tp0 = tp1 = 0;
		for(int k = 0;k < 16;++k){ tp0 |= (unsigned long long)Tq[k] << (4*k); tp1 |= (unsigned long long)Tq[16 + k] << (4*k); }
	}

	__device__ __forceinline__ static int code_at(unsigned long long p0, unsigned long long p1, int k)
	{
		return (int)(((k < 16) ? (p0 >> (4*k)) : (p1 >> (4*(k - 16)))) & 0xF);
	}

	// align_dimer / align_hairpin (nuc_cruc.cpp:347-541, :543-816; per cell :381-511 == :658-786) by the whole wave: lane l owns column
	// l + 1 and the wave sweeps the anti-diagonals i + j = d, whose cells are independent.  A cell's neighbours
	// are the lane's own cell of the previous diagonal (i-1, j) and lane l-1's cells of the previous two,
	// (i, j-1) and (i-1, j-1): three wave shifts per step, nothing read back from memory.  QL + TL - 1 steps
	// instead of QL*TL cells.  Rows 1..rows; row i has n - (i-1)*shrink columns (shrink 0: dimer, 1: hairpin).
	// Every lane of the wave must call this; returns the maximum M to all lanes.
	__device__ int fill_wave(const unsigned char *Q, int QL, const unsigned char *Tq, int rows, int n, int shrink)
	{
		const int lane = (int)(threadIdx.x & 63u);
		const int jc = lane + 1;
		unsigned long long qp0, qp1, tp0, tp1;
		pack_codes(Q, qp0, qp1);
		pack_codes(Tq, tp0, tp1);
		const int tb = code_at(tp0, tp1, lane & 31);
		const int ptb = (lane == 0) ? (int)bGAP : code_at(tp0, tp1, (lane - 1) & 31);
		int pM = -1, pIq = -1, pIt = -1;                 // own cell of the previous diagonal: (i-1, jc)
		int aM = -1, aIq = -1, aIt = -1;                 // lane-1's cell two diagonals back:  (i-1, jc-1)
		int best = -1;
		// The seven table entries of a cell depend on the codes only, not on the DP values: the one that does not depend on the row is
		// read once, the other six are requested a diagonal ahead (before this diagonal's stores), so that their LDS latency runs
		// beside the arithmetic instead of in front of it.
		const int g_ext_q = dg[PAIR(ptb, bGAP)*49 + PAIR(tb, bGAP)];
		struct Costs { int m_diag, m_left, m_up, q_ins, t_ins, t_ext; };
		auto costs = [&](int d) -> Costs {
			const int i = d - jc;
			const bool first_row = (i == 1);
			const int qb = code_at(qp0, qp1, (QL - i) & 31);
			const int pqb = first_row ? (int)bGAP : code_at(qp0, qp1, (QL - i + 1) & 31);
			const int cur = PAIR(tb, qb), curt = PAIR(bGAP, qb);
			Costs c;
			c.m_diag = dg[PAIR(ptb, pqb)*49 + cur];
			c.m_left = dg[PAIR(ptb, bGAP)*49 + cur];
			c.m_up = dg[PAIR(bGAP, pqb)*49 + cur];
			c.q_ins = dg[PAIR(ptb, qb)*49 + PAIR(tb, bGAP)];
			c.t_ins = dg[PAIR(tb, pqb)*49 + curt];
			c.t_ext = dg[PAIR(bGAP, pqb)*49 + curt];
			return c;
		};
		Costs c = costs(2);
		for(int d = 2;d <= rows + n;++d){
			// lane-1's (i, jc-1): a wave shift through the DPP path (no LDS round trip); lane 0 keeps the -1 it passes in
			const int cM = __builtin_amdgcn_update_dpp(-1, pM, 0x138, 0xf, 0xf, false);
			const int cIq = __builtin_amdgcn_update_dpp(-1, pIq, 0x138, 0xf, 0xf, false);
			const int cIt = __builtin_amdgcn_update_dpp(-1, pIt, 0x138, 0xf, 0xf, false);
			const Costs nx = costs(d + 1);
			const int i = d - jc;
			const bool valid = (i >= 1) && (i <= rows) && (jc <= n - (i - 1)*shrink);
			const bool first_row = (i == 1);
			const int AM = first_row ? -1 : aM, AIq = first_row ? -1 : aIq, AIt = first_row ? -1 : aIt;
			const int BM = first_row ? -1 : pM, BIt = first_row ? -1 : pIt;
			const int dg1 = step(AM, c.m_diag);
			const int dg2 = step(AIq, c.m_left);
			const int dg3 = step(AIt, c.m_up);
			int M; unsigned Mt;
			if(dg1 >= dg2){
				if(dg1 >= dg3){ M = dg1; Mt = T_DIAG; if(dg1 == dg2) Mt |= T_LEFT; if(dg1 == dg3) Mt |= T_UP; }
				else{ M = dg3; Mt = T_UP; }
			}
			else{
				if(dg2 >= dg3){ M = dg2; Mt = T_LEFT; if(dg2 == dg3) Mt |= T_UP; }
				else{ M = dg3; Mt = T_UP; }
			}
			int ins = step(cM, c.q_ins);
			int ext = step(cIq, g_ext_q);
			int Iq; unsigned Iqt;
			if(ins >= ext){ Iq = ins; Iqt = T_DIAG; if(ins == ext) Iqt |= T_LEFT; }
			else{ Iq = ext; Iqt = T_LEFT; }
			ins = step(BM, c.t_ins);
			ext = step(BIt, c.t_ext);
			int It; unsigned Itt;
			if(ins >= ext){ It = ins; Itt = T_DIAG; if(ins == ext) Itt |= T_UP; }
			else{ It = ext; Itt = T_UP; }
			aM = cM; aIq = cIq; aIt = cIt;
			if(valid){
				const int x = i*STRIDE + jc;
				mx.M[x*LS] = M;
				mx.tr[x*LS] = (unsigned short)(Mt | (Iqt << 4) | (Itt << 8) | ((Iq < 0) ? 0x1000u : 0u) | ((It < 0) ? 0x2000u : 0u));
				best = max(best, M);
				pM = M; pIq = Iq; pIt = It;
			}
			c = nx;
		}
		for(int off = 32;off > 0;off >>= 1) best = max(best, __shfl_xor(best, off));
		return best;
	}

	__device__ static bool path_split(unsigned m) { return ((m & 1) + ((m & 2) >> 1) + ((m & 4) >> 2)) > 1; }

	// boundary-aware reads for the trace back (row 0 / column 0 are never filled)
	__device__ int cellM(int c) const { return ((c/STRIDE) == 0 || (c % STRIDE) == 0) ? -1 : mx.getM(c); }
	__device__ bool cellIqNeg(int c) const { return ((c/STRIDE) == 0 || (c % STRIDE) == 0) ? true : mx.negIq(c); }
	__device__ bool cellItNeg(int c) const { return ((c/STRIDE) == 0 || (c % STRIDE) == 0) ? true : mx.negIt(c); }
	__device__ unsigned cellTrace(int c, int which) const { return ((c/STRIDE) == 0 || (c % STRIDE) == 0) ? (unsigned)T_INVALID : mx.trace(c, which); }

	// NucCruc::trace_back, nuc_cruc.cpp:1262-1471.  Returns false on a malformed trace (never for DP-made matrices).
	__device__ bool trace_back(int cell, Branch *stack, int &n_stack, int &zero_count, Align &a,
		const unsigned char *Q, int QL, const unsigned char *Tq)
	{
		int last_i = cell/STRIDE, last_j = cell % STRIDE;
		a.first_q = QL - last_i; a.first_t = last_j - 1;
		int truncate_at_zero = 0;
		bool count_zeros = false;
		if(zero_count < 0){ zero_count = 0; count_zeros = true; }
		else{ truncate_at_zero = zero_count--; }
		int id = -1;
		unsigned mask = T_DIAG;
		while(true){
			bool ok = true;
			unsigned local;
			if(path_split(mask)){
				int k = 0;
				for(;k < n_stack;++k){ if(stack[k].id == id) break; }
				if(k == n_stack){
					if(n_stack >= 4*MAXL) return false;
					stack[k].id = (unsigned short)id;
					stack[k].cur = (mask & T_DIAG) ? T_DIAG : ((mask & T_UP) ? T_UP : T_LEFT);
					++n_stack;
				}
				local = stack[k].cur;
			}
			else local = mask;
			if(a.tail >= ALN - 1) return false;
			if(local == T_DIAG){
				if(last_i > QL || last_j < 1) ok = false;
				else{
					const int m = cellM(cell);
					if(m < 0) ok = false;
					else if(m == 0){
						if(count_zeros) ++zero_count;
						else{ --truncate_at_zero; if(truncate_at_zero == 0) ok = false; }
					}
					a.qa[a.tail] = Q[QL - last_i];      // last_i == 0 reads Q[QL], defined as E (DESIGN.md)
					a.ta[a.tail] = Tq[last_j - 1];
					++a.tail;
					a.last_q = QL - last_i; a.last_t = last_j - 1;
					id = cell*3 + 0; mask = cellTrace(cell, 0);
					--last_i; --last_j;
				}
			}
			else if(local == T_LEFT){
				if(last_j < 1) ok = false;
				else{
					if(cellIqNeg(cell)) ok = false;
					a.qa[a.tail] = bGAP; a.ta[a.tail] = Tq[last_j - 1]; ++a.tail;
					a.last_q = QL - last_i + 1; a.last_t = last_j - 1;
					id = cell*3 + 1; mask = cellTrace(cell, 1);
					--last_j;
				}
			}
			else if(local == T_UP){
				if(last_i > QL) ok = false;
				else{
					if(cellItNeg(cell)) ok = false;
					a.qa[a.tail] = Q[QL - last_i]; a.ta[a.tail] = bGAP; ++a.tail;
					a.last_q = QL - last_i; a.last_t = last_j;
					id = cell*3 + 2; mask = cellTrace(cell, 2);
					--last_i;
				}
			}
			else return false;
			if(!ok) break;
			if(last_i < 0 || last_j < 0) return false;
			cell = last_i*STRIDE + last_j;
		}
		return true;
	}

	__device__ bool next_trace(Branch &b) const                                 // trace_branch::next_trace, nuc_cruc.h:287-304
	{
		const int cell = b.id/3, which = b.id % 3;
		const unsigned mask = cellTrace(cell, which);
		unsigned cur = b.cur;
		while((cur = (cur << 1) & 0xFF) < T_INVALID && cur != 0){
			if(cur & mask){ b.cur = (unsigned char)cur; return true; }
		}
		return false;
	}

	__device__ void trim_frayed(Align &a) const                                 // nuc_cruc.cpp:868-903
	{
		while(a.size() > 0 && !c_wc[PAIR(a.qa[a.tail - 1], a.ta[a.tail - 1])]){
			if(a.qa[a.tail - 1] < bE) --a.last_q;
			if(a.ta[a.tail - 1] < bE) ++a.last_t;
			--a.tail;
		}
		while(a.size() > 0 && !c_wc[PAIR(a.qa[a.head], a.ta[a.head])]){
			if(a.qa[a.head] < bE) ++a.first_q;
			if(a.ta[a.head] < bE) --a.first_t;
			++a.head;
		}
	}

	__device__ void advance_stack(Branch *stack, int &n_stack, int &zero_count) const   // nuc_cruc.cpp:907-915
	{
		if(zero_count == 0 && n_stack > 0){
			while(n_stack > 0 && !next_trace(stack[n_stack - 1])) --n_stack;
			zero_count = -1;
		}
	}

	template<class B> __device__ void keep_if_better(B &bst, float &best_dg, const Align &loc) const  // :1009-1016
	{
		const float local_dg = loc.dH - TARGET_T*loc.dS;
		if(!bst.valid || local_dg < best_dg){
			bst.dH = loc.dH; bst.dS = loc.dS; bst.tm = loc.tm; bst.valid = true;   // only the energies are reported
			best_dg = local_dg;
		}
	}

	__device__ static bool non_virtual(int p) { return (p % NB < bE) && (p/NB < bE); }
	__device__ static bool has_gap(int p) { return (p % NB == bGAP) || (p/NB >= bGAP); }

	__device__ bool has_AT_initiation(const Align &a, int k) const              // nuc_cruc.cpp:2747-2764
	{
		do{ --k; } while(k != a.head && (a.qa[k] == bGAP || a.ta[k] == bGAP));
		const int bp = PAIR(a.qa[k], a.ta[k]);
		return bp == pAT || bp == pTA;
	}

	// NucCruc::evaluate_alignment, nuc_cruc.cpp:1473-2137.  Accumulation order of dH / dS is the reference's.
	__device__ bool evaluate(Align &a, int mode) const
	{
		int terminal = p__, lastlast = p__, last = p__, cur = p__;
		if(mode != HAIRPIN){
			a.dH = PCR_INIT_H;
			a.dS = PCR_INIT_S + ((mode == HOMO_DIMER) ? PCR_SYMMETRY_S : 0.0f);
		}
		unsigned n_qgap = 0, n_tgap = 0, n_mm = 0, num_base = 0;
		bool terminal_5 = false;
		int k = a.head;
		cur = PAIR(a.qa[k], a.ta[k]);
		if(c_wc[cur]){
			terminal_5 = true;
			if(cur == pAT || cur == pTA){ a.dH += PCR_AT_H; a.dS += PCR_AT_S; }
		}
		num_base += (a.qa[k] < bE) ? 1 : 0;
		num_base += (a.ta[k] < bE) ? 1 : 0;
		++k;
		unsigned idx = 1;
		const unsigned asize = (unsigned)a.size();
		for(;k != a.tail;++k, ++idx){
			lastlast = last; last = cur; cur = PAIR(a.qa[k], a.ta[k]);
			const bool align_start = (idx == 1), align_stop = (idx == asize - 1);
			const int qk = a.qa[k], tk = a.ta[k];
			const bool in_loop = (qk == bGAP) || (tk == bGAP) || (!c_wc[last] && !c_wc[cur]);
			if(!in_loop){
				if(align_start && !c_wc[last] && non_virtual(last)){
					const int tq = last/NB, tt = last % NB;
					int tp = PAIR(tq, bE);
					a.dH += c_H[tp*49 + cur]; a.dS += c_S[tp*49 + cur];
					tp = PAIR(bE, tt);
					a.dH += c_H[tp*49 + cur]; a.dS += c_S[tp*49 + cur];
				}
				else if(align_stop && !c_wc[cur] && non_virtual(cur)){
					int tp = PAIR(qk, bE);
					a.dH += c_H[last*49 + tp]; a.dS += c_S[last*49 + tp];
					tp = PAIR(bE, tk);
					a.dH += c_H[last*49 + tp]; a.dS += c_S[last*49 + tp];
				}
				else{ a.dH += c_H[last*49 + cur]; a.dS += c_S[last*49 + cur]; }
				num_base += (qk < bE) ? 1 : 0;
				num_base += (tk < bE) ? 1 : 0;
			}
			if(c_wc[cur]){
				terminal = cur;
				if(!terminal_5){
					terminal_5 = true;
					if(cur == pAT || cur == pTA){ a.dH += PCR_AT_H; a.dS += PCR_AT_S; }
				}
				const unsigned max_gap = max(n_qgap, n_tgap);
				if(n_mm > 1 || (max_gap > 0 && n_mm == 1)){
					const unsigned gap_diff = (n_qgap > n_tgap) ? n_qgap - n_tgap : n_tgap - n_qgap;
					const unsigned loop_size = n_mm*2 + gap_diff;
					if(loop_size == 2 && (last == pGT || last == pTG) && (lastlast == pGT || lastlast == pTG)){
						a.dH += c_H[lastlast*49 + last]; a.dS += c_S[lastlast*49 + last];
						num_base += 2;
					}
					else{
						a.dS += c_loop_S[loop_size];
						a.dS += (float)gap_diff*PCR_ASYM_LOOP_S;
						int rq = k - 1, rt = k - 1;
						a.dH -= c_H[last*49 + cur]; a.dS -= c_S[last*49 + cur];
						if(!has_gap(last)){ a.dH += c_H[last*49 + cur]; a.dS += c_S[last*49 + cur]; }
						else{
							int mm = p__;
							if(last/NB == bGAP){
								while(true){
									if(a.qa[rq] < bE){ mm = PAIR(a.qa[rq], last % NB); break; }
									if(rq == a.head) break;
									--rq;
								}
							}
							else{
								while(true){
									if(a.ta[rt] < bE){ mm = PAIR(last/NB, a.ta[rt]); break; }
									if(rt == a.head) break;
									--rt;
								}
							}
							a.dH += c_H[mm*49 + cur]; a.dS += c_S[mm*49 + cur];
						}
						int lq = k - 1, lt = k - 1;
						while(true){
							const int pm = PAIR(a.qa[lq], a.ta[lt]);
							if(c_wc[pm]){
								++lq; ++lt;
								if(a.qa[lq] != bGAP && a.ta[lt] != bGAP){
									const int mm = PAIR(a.qa[lq], a.ta[lt]);
									a.dH -= c_H[pm*49 + mm]; a.dS -= c_S[pm*49 + mm];
								}
								num_base += 2;
								while(a.qa[lq] == bGAP && lq < a.tail) ++lq;
								while(a.ta[lt] == bGAP && lt < a.tail) ++lt;
								const int mm = PAIR(a.qa[lq], a.ta[lt]);
								a.dH += c_H[pm*49 + mm]; a.dS += c_S[pm*49 + mm];
								break;
							}
							if(lq == a.head) break;
							--lq; --lt;
						}
						if(rq != lq) ++num_base;
						if(rt != lt) ++num_base;
					}
				}
				else if(n_qgap || n_tgap){
					const unsigned bulge = (n_qgap > n_tgap) ? n_qgap : n_tgap;
					if(bulge == 1){ a.dH += c_H[lastlast*49 + cur]; a.dS += c_S[lastlast*49 + cur]; }
					a.dS += c_bulge_S[bulge];
					if(bulge != 1 && (qk == bA || qk == bT)) a.dS += PCR_BULGE_AT_S;
					if(bulge != 1 && has_AT_initiation(a, k)) a.dS += PCR_BULGE_AT_S;
				}
				n_qgap = n_tgap = 0; n_mm = 0;
			}
			else n_mm += (qk < bE && tk < bE) ? 1 : 0;
			n_qgap += (qk == bGAP) ? 1 : 0;
			n_tgap += (tk == bGAP) ? 1 : 0;
		}
		if(terminal == pAT || terminal == pTA){ a.dH += PCR_AT_H; a.dS += PCR_AT_S; }
		if(a.dH >= 0.0f) return false;
		a.dS += __fmul_rn(__fmul_rn(PCR_SALT, (0.5f*(float)num_base - 1.0f)), log_na);                 // :2108
		float tm;
		if(mode == HAIRPIN) tm = __fdiv_rn(a.dH, a.dS) - ZERO_C;                                       // :2126
		else tm = __fdiv_rn(a.dH, (__fmul_rn(GAS_R, log_strand) + a.dS)) - ZERO_C;                      // :2129
		a.tm = fmaxf(0.0f, tm);
		return true;
	}

	__device__ int find_loop_index(const unsigned char *Q, int start, int len) const   // nuc_cruc.cpp:2478-2728
	{
		unsigned v = 0;
		for(int i = 0;i < len;++i){ if(Q[start + i] > bT) return -1; v = v*4 + Q[start + i]; }
		const unsigned key = ((unsigned)len << 16) | v;
		for(int i = 0;i < 131;++i){ if(c_special_key[i] == key) return i; }   // exact lookup == the sorted-prefix scan of the reference
		return -1;
	}

	__device__ bool evaluate_hairpin(Align &a) const                            // nuc_cruc.cpp:2139-2232
	{
		const int last_3 = a.first_q, last_5 = a.first_t;
		const unsigned loop_len = (unsigned)(last_3 - last_5 - 1);
		if(last_5 < 0 || last_3 >= qlen || last_3 <= last_5 || loop_len > 128) return false;
		a.dH = 0.0f; a.dS = 0.0f;
		a.dS += c_hairpin_S[loop_len];
		const int lastp = PAIR(q[last_5], q[last_3]);
		if(loop_len == 3){
			const int li = find_loop_index(q, last_5, 5);
			if(li >= 0){ a.dH += c_special_H[li]; a.dS += c_special_S[li]; }
			if(lastp == pAT || lastp == pTA) a.dS += PCR_BULGE_AT_S;
		}
		else{
			if(loop_len == 4){
				const int li = find_loop_index(q, last_5, 6);
				if(li >= 0){ a.dH += c_special_H[li]; a.dS += c_special_S[li]; }
			}
			const int curp = PAIR(q[last_5 + 1], q[last_3 - 1]);
			a.dH += c_H[lastp*49 + curp]; a.dS += c_S[lastp*49 + curp];
		}
		return evaluate(a, HAIRPIN);
	}

	// enumerate_dimer_alignments, nuc_cruc.cpp:818-1019
	template<class B> __device__ bool enumerate_dimer(int cell, B &bst, Align &loc, Branch *stack, const unsigned char *Q, int QL,
		const unsigned char *Tq, int TL, int mode)
	{
		bool first = true;
		int n_stack = 0, zero_count = -1;
		unsigned trace_count = 0;
		float best_dg = bst.dH - TARGET_T*bst.dS;
		while(true){
			if(!first && n_stack == 0 && zero_count <= 0) break;
			if(MAX_PATH_ENUM < trace_count) break;
			++trace_count;
			first = false;
			loc.reset();
			if(!trace_back(cell, stack, n_stack, zero_count, loc, Q, QL, Tq)) return false;
			trim_frayed(loc);
			advance_stack(stack, n_stack, zero_count);
			if(loc.size() == 0) continue;
			if(loc.first_q != 0 || loc.first_t != TL - 1){
				--loc.head;
				if(loc.first_q == 0) loc.qa[loc.head] = bE;
				else{ --loc.first_q; loc.qa[loc.head] = Q[loc.first_q]; }
				if(loc.first_t == TL - 1) loc.ta[loc.head] = bE;
				else{ ++loc.first_t; loc.ta[loc.head] = Tq[loc.first_t]; }
			}
			if(loc.last_q != QL - 1 || loc.last_t != 0){
				if(loc.last_q == QL - 1) loc.qa[loc.tail] = bE;
				else{ ++loc.last_q; loc.qa[loc.tail] = Q[loc.last_q]; }
				if(loc.last_t == 0) loc.ta[loc.tail] = bE;
				else{ --loc.last_t; loc.ta[loc.tail] = Tq[loc.last_t]; }
				++loc.tail;
			}
			if(loc.size() < 3) continue;
			if(evaluate(loc, mode)) keep_if_better(bst, best_dg, loc);
		}
		return true;
	}

	// enumerate_hairpin_alignments, nuc_cruc.cpp:1021-1260
	template<class B> __device__ bool enumerate_hairpin(int cell, B &bst, Align &loc, Branch *stack, const unsigned char *Q, int QL)
	{
		bool first = true;
		int n_stack = 0, zero_count = -1;
		unsigned trace_count = 0;
		float best_dg = bst.dH - TARGET_T*bst.dS;
		while(true){
			if(!first && n_stack == 0 && zero_count <= 0) break;
			if(MAX_PATH_ENUM < trace_count) break;
			++trace_count;
			first = false;
			loc.reset();
			if(!trace_back(cell, stack, n_stack, zero_count, loc, Q, QL, Q)) return false;
			trim_frayed(loc);
			advance_stack(stack, n_stack, zero_count);
			if(loc.size() == 0) continue;
			if(loc.size() >= 3 && evaluate_hairpin(loc)) keep_if_better(bst, best_dg, loc);
			if(loc.last_t != 0 || loc.last_q != QL - 1){
				if(loc.last_t == 0) loc.ta[loc.tail] = bE;
				else{ --loc.last_t; loc.ta[loc.tail] = Q[loc.last_t]; }
				if(loc.last_q == QL - 1) loc.qa[loc.tail] = bE;
				else{ ++loc.last_q; loc.qa[loc.tail] = Q[loc.last_q]; }
				++loc.tail;
			}
			const int asize = loc.size();
			if(asize < 3) continue;
			if(evaluate_hairpin(loc)) keep_if_better(bst, best_dg, loc);
			if(asize <= 3) continue;
			const int lastp = PAIR(q[loc.first_t], q[loc.first_q]);
			if(lastp == pGC || lastp == pCG) continue;
			++loc.first_q; --loc.first_t;
			++loc.head;
			if(evaluate_hairpin(loc)) keep_if_better(bst, best_dg, loc);
		}
		return true;
	}

	// The perfect-match duplex (nuc_cruc.h:723-759) by the whole wave (every lane calls it): evaluate() on a gapless Watson-Crick alignment of q with its complement
	// reduces to the initiation terms, the terminal A-T terms, one nearest-neighbour term per step -- added in the alignment's
	// order -- and the salt term over 2*qlen bases (nuc_cruc.cpp:1473-2137 with in_loop false, no gap, no mismatch on every step).
	// The lanes fetch the steps' table entries side by side (one memory latency instead of one per step); the sums are formed in
	// the reference's order on every lane alike.  dH >= 0: evaluate() returns before the salt term and Tm stays 0 (Align::reset).
	__device__ float tm_pm_duplex_wave(float &dH_out, float &dS_out) const
	{
		const int lane = (int)(threadIdx.x & 63u);
		const int QLu = __builtin_amdgcn_readfirstlane(qlen);
		const int k0 = min(lane, QLu - 1), k1 = min(lane + 1, QLu - 1);
		const int p0 = PAIR(q[k0], 3 - q[k0]), p1 = PAIR(q[k1], 3 - q[k1]);
		const float h = c_H[p0*49 + p1], sv = c_S[p0*49 + p1];
		float dH = PCR_INIT_H, dS = PCR_INIT_S + 0.0f;
		const int first = __builtin_amdgcn_readfirstlane(p0);
		if(first == pAT || first == pTA){ dH += PCR_AT_H; dS += PCR_AT_S; }
		for(int k = 0;k + 1 < QLu;++k){
			dH += __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, h), k));
			dS += __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, sv), k));
		}
		if(QLu >= 2){
			const int terminal = __builtin_amdgcn_readlane(p0, QLu - 1);
			if(terminal == pAT || terminal == pTA){ dH += PCR_AT_H; dS += PCR_AT_S; }
		}
		float tm = 0.0f;
		if(!(dH >= 0.0f)){
			dS += __fmul_rn(__fmul_rn(PCR_SALT, (0.5f*(float)(unsigned)(2*QLu) - 1.0f)), log_na);
			tm = fmaxf(0.0f, __fdiv_rn(dH, (__fmul_rn(GAS_R, log_strand) + dS)) - ZERO_C);
		}
		dH_out = dH; dS_out = dS;
		return tm;
	}
};

struct Job {            // one lane of work
	unsigned char q[MAXL], t[MAXL];
	unsigned char qlen, tlen, mode /* 0: oligo (duplex + hairpin [+ homodimer]); 1: heterodimer q x t */, check_homo;
	float log_strand;
};

constexpr unsigned char JOB_PACKED = 0x80;   // flag in Job::mode (oligo jobs only, tlen = 0): q[0..15] = the oligo's slot masks A, C, G, T (u32 each), t[0] = its first occupied slot

struct JobOut { float tm_pm, dH_pm, dS_pm, tm_hairpin, tm_dimer; unsigned int status; };   // status bit0: internal error

// ONE job per wave, whatever the batch size.  A lane's DP is a chain of dependent cell updates and a wave issues an
// instruction every few cycles whether one lane works or 64, so the wave fills the matrices together along
// anti-diagonals (Engine::fill_wave), finds the maximum cells together and walks their trace-backs on WAVE_PAR lanes.
// Matrices, sequences, alignments, branch stacks and the cell masks live in LDS; the kernel uses no scratch memory.
// (A 64-jobs-per-wave form with the matrices in a global slab -- 1 240 B of scratch per lane -- existed until round 2;
// measured on the box it lost at every batch size: 20 000 oligos 10.7 vs 1.45 ms, 100 000 40.3 vs 6.6 ms.)
//
// A job is a chain of dependent instructions and LDS round trips (table lookups, the pointer-chasing trace-backs), so what a CU
// gets done is set by how many waves it holds.  r02 ran one wave per block with 38 KB of LDS each = 4 waves per CU, one per SIMD,
// 47 % of their cycles parked on s_waitcnt with nothing else to issue (profiles/r03_secondary_pmc.md): 36 ns per job.  Now a
// block is THERMO_WAVES independent waves around ONE copy of the dG table (9.6 KB), each with an 11.6 KB slab: of the DP planes only
// M and one 16-bit plane are stored (Matrix), the running best alignment keeps only its energies (nothing else of it is ever
// read), a branch point takes 2 bytes, the maximum cells are a bit mask per row instead of a list, and the perfect-match duplex
// is summed by the wave from table entries its lanes fetch side by side (one lane walking evaluate() was a quarter of a job).
// Measured (20 000 is_valid oligos = 40 000 jobs): 4 waves per CU 1.46 ms, 7 waves 0.72 ms, 12 waves 0.47 ms; a job's own latency
// (77 000 - 86 000 cycles, PCRAMP_THERMO_TIMING=1: fill 40 %, trace-backs 43 %) hardly moves with the number of waves beside it.
constexpr int THERMO_WAVES = 12;
constexpr int THERMO_THREADS = 64*THERMO_WAVES;

// The cells holding the maximum are enumerated independently of each other, and the reference keeps the first
// alignment with the lowest dG in row-major cell order (keep_if_better: the first valid one, then strictly
// better ones only).  So WAVE_PAR lanes take the cells round-robin, each keeping its own best by the same rule
// and the cell that produced it, and lane 0 merges: lowest dG, earliest cell on a tie -- the alignment the
// sequential sweep ends with.  (With a low maximum, dozens of cells tie; this part was 2/3 of a job's latency.)
constexpr int WAVE_PAR = 8;
struct Best { bool valid; float dH, dS, tm; __device__ void reset() { valid = false; dH = dS = tm = 0.0f; } };   // what keep_if_better keeps
struct ParLane { Align loc; Best best; Branch stack[4*MAXL]; int win; unsigned bad; };

struct WaveSlab {
	int si[NCELL];                        // M
	unsigned short ss[NCELL];             // trace masks + the signs of Iq, It (Matrix)
	unsigned int rowmask[STRIDE + 3];     // bit l of [i]: cell (i, l + 1) holds the maximum
	unsigned char q[MAXL + 4], t[MAXL + 4];
	ParLane par[WAVE_PAR];
};
constexpr size_t THERMO_LDS = 49*49*sizeof(int) + THERMO_WAVES*sizeof(WaveSlab);
static_assert(THERMO_LDS <= 160*1024 - 512, "a block of THERMO_WAVES waves must fit one CU's LDS");

// every lane of the wave calls this (a row per step, a column per lane); returns the number of maximum cells
__device__ __forceinline__ int collect_rows(const Engine<1> &e, int rows, int n, int shrink, int mxs, unsigned int *rowmask)
{
	const int lane = (int)(threadIdx.x & 63u), jc = lane + 1;
	unsigned mine = 0;
	int total = 0;
	for(int i = 1;i <= rows;++i){
		const bool hit = (jc <= n - (i - 1)*shrink) && (jc <= MAXL) && (e.mx.getM(i*STRIDE + min(jc, MAXL)) == mxs);
		const unsigned m = (unsigned)__ballot(hit);                  // columns 1 .. 32 = lanes 0 .. 31
		if(lane == i) mine = m;
		total += __popc(m);
	}
	if(lane <= MAXL) rowmask[lane] = mine;                           // (rows beyond `rows`, and row 0: empty)
	return total;
}

template<bool HAIRPIN> __device__ float enumerate_parallel(Engine<1> &e, ParLane *par, const unsigned int *rowmask, int rows, bool homo,
	unsigned &status)
{
	const int lane = (int)(threadIdx.x & 63u);
	if(lane < WAVE_PAR){
		ParLane &L = par[lane];
		L.best.reset(); L.win = -1; L.bad = 0;
		int k = 0;                                                     // ordinal of the cell in row-major order (max_ptr's, nuc_cruc.cpp:515-536)
		bool go = true;
		for(int i = 1;i <= rows && go;++i){
			for(unsigned m = rowmask[i];m && go;m &= m - 1u, ++k){
				if((k % WAVE_PAR) != lane) continue;
				const int cell = i*STRIDE + (int)__builtin_ctz(m) + 1;
				const bool was = L.best.valid;
				const float before = L.best.dH - TARGET_T*L.best.dS;
				const bool ok = HAIRPIN ? e.enumerate_hairpin(cell, L.best, L.loc, L.stack, e.q, e.qlen)
					: e.enumerate_dimer(cell, L.best, L.loc, L.stack, e.q, e.qlen, homo ? e.q : e.t, homo ? e.qlen : e.tlen, homo ? HOMO_DIMER : HETERO_DIMER);
				if(!ok){ L.bad = 1; go = false; break; }
				const float after = L.best.dH - TARGET_T*L.best.dS;
				if(L.best.valid && (!was || after < before)) L.win = k;
			}
		}
	}
	wave_sync();
	float tm = 0.0f;
	if(lane == 0){
		// (k_site_tm, pcr_site_tm.inc, and pdim_winner, pcr_pool_dimers.inc, repeat this merge to take the winner's dH and dS: change the three together)
		int win = -1;
		float wdg = 0.0f;
		for(int l = 0;l < WAVE_PAR;++l){
			const ParLane &L = par[l];
			if(L.bad) status |= 1u;
			if(L.win < 0) continue;
			const float dgl = L.best.dH - TARGET_T*L.best.dS;
			if(win < 0 || dgl < wdg || (dgl == wdg && L.win < win)){ win = L.win; wdg = dgl; tm = L.best.tm; }
		}
	}
	return tm;
}

// The validity form of the kernel (the local search's is_valid of thousands of trial words per iteration, most of them
// degenerate): one packed record per WORD, a map job -> (record, expansion index) beside it, and the verdict reduced on the
// device -- word_bad[record] becomes non-zero if any expansion leaves the Tm range or exceeds the hairpin limit
// (valid_pcr.cpp:19-31), 2 on an internal error.  The host then neither spells the expansions (72 bytes each) nor reads
// 24 bytes of results per expansion back.  map == nullptr: the plain form.
struct ThermoValid { const uint2 *map; unsigned int *word_bad; float tm_min, tm_max, max_hairpin; };

// n_mirror: jobs n_jobs .. n_jobs + n_mirror - 1 are the homodimer halves (mode 2) of the oligo jobs 0 .. n_mirror - 1, read from
// the same records (the host neither copies nor uploads them twice); those oligo jobs then skip their own homodimer test.
__global__ __launch_bounds__(THERMO_THREADS) void k_thermo_wave(const Job *__restrict__ jobs, unsigned n_jobs, unsigned n_mirror, const int *__restrict__ dg_global,
	float log_na, JobOut *__restrict__ out, ThermoValid V, unsigned long long *__restrict__ dbg_cycles)
{
	extern __shared__ int th_lds[];                                                // dg [49*49] | THERMO_WAVES slabs
	int *const dg = th_lds;
	const unsigned wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
	WaveSlab &w = ((WaveSlab *)(th_lds + 49*49))[wave];
	for(int i = threadIdx.x;i < 49*49;i += THERMO_THREADS) dg[i] = dg_global[i];
	__syncthreads();                                                               // the only workgroup barrier: from here on every wave is on its own
	const bool lead = (lane == 0);
	Engine<1> e;
	e.dg = dg; e.log_na = log_na;
	e.q = w.q; e.t = w.t;
	e.mx.M = w.si;
	e.mx.tr = w.ss;
	unsigned long long t_fill = 0, t_collect = 0, t_enum = 0, t_other = 0, t_mark = dbg_cycles ? (unsigned long long)clock64() : 0;
	auto lap = [&](unsigned long long &acc){ if(dbg_cycles){ const unsigned long long now = (unsigned long long)clock64(); acc += now - t_mark; t_mark = now; } };
	for(unsigned j = blockIdx.x*THERMO_WAVES + wave;j < n_jobs + n_mirror;j += gridDim.x*THERMO_WAVES){   // uniform per wave: the whole wave takes the same jobs
		// (read in place: a private copy of the 72-byte job indexed by the lane would live in scratch memory)
		const bool mirrored = j >= n_jobs;
		unsigned rec = mirrored ? j - n_jobs : j, expansion = 0;
		if(V.map){
			const uint2 m = V.map[j]; rec = m.x; expansion = m.y;
			if(expansion && __hip_atomic_load(&V.word_bad[rec], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) continue;   // an earlier expansion already failed (uniform: the whole wave skips)
		}
		const Job *const jp = jobs + rec;
		struct { unsigned char qlen, tlen, mode, check_homo; } jb = {jp->qlen, jp->tlen, jp->mode, jp->check_homo};
		const bool packed = (jb.mode & JOB_PACKED) != 0;                           // q holds the oligo's four slot masks, not codes
		jb.mode &= (unsigned char)~JOB_PACKED;
		if(mirrored) jb.mode = 2;
		else if(j < n_mirror) jb.check_homo = 0;
		e.log_strand = jp->log_strand; e.qlen = jb.qlen; e.tlen = jb.tlen;
		if(lane <= MAXL){
			const int i = (int)lane;
			unsigned char qc = jp->q[i & (MAXL - 1)];
			if(packed){                                                              // slot first + i of the masks {A, C, G, T}
				const unsigned int *pl = (const unsigned int *)jp->q;
				const unsigned first = jp->t[0];
				auto base_set = [&](unsigned slot) -> unsigned { const unsigned b = slot & 31u; return ((pl[0] >> b) & 1u) | (((pl[1] >> b) & 1u) << 1) | (((pl[2] >> b) & 1u) << 2) | (((pl[3] >> b) & 1u) << 3); };
				// expansion e of a degenerate oligo: mixed radix over its slots, slot k's digit picks among its bases (lowest first)
				unsigned div = 1;
				for(int k = 0;k < i && k < (int)jb.qlen;++k) div *= (unsigned)__popc(base_set(first + k));
				unsigned set = base_set(first + i);
				const unsigned d = max((unsigned)__popc(set), 1u);
				for(unsigned skip = (expansion/div) % d;skip;--skip) set &= set - 1u;     // drop the lower bases
				qc = (unsigned char)(set ? (unsigned)__ffs(set) - 1u : 0u);
			}
			w.q[i] = (i < jb.qlen) ? qc : (unsigned char)bE;                         // "one past the end" is the non-pairing code E (see DESIGN.md)
			w.t[i] = (i < jb.tlen) ? jp->t[i & (MAXL - 1)] : (unsigned char)bE;
		}
		wave_sync();
		JobOut r; r.tm_pm = r.dH_pm = r.dS_pm = r.tm_hairpin = r.tm_dimer = 0.0f; r.status = 0;
		lap(t_other);
		if(jb.mode == 0){
			r.tm_pm = e.tm_pm_duplex_wave(r.dH_pm, r.dS_pm);
			const int max_stem = e.qlen - 4;
			lap(t_other);
			int mxs = e.fill_wave(e.q, e.qlen, e.q, max_stem, max_stem, 1);
			wave_sync();
			lap(t_fill);
			collect_rows(e, max_stem, max_stem, 1, mxs, w.rowmask);
			wave_sync();
			lap(t_collect);
			r.tm_hairpin = enumerate_parallel<true>(e, w.par, w.rowmask, max_stem, false, r.status);
			lap(t_enum);
			if(jb.check_homo){
				wave_sync();                                                         // the trace-back lanes are done with the hairpin matrices
				mxs = e.fill_wave(e.q, e.qlen, e.q, e.qlen, e.qlen, 0);
				wave_sync();
				lap(t_fill);
				collect_rows(e, e.qlen, e.qlen, 0, mxs, w.rowmask);
				wave_sync();
				lap(t_collect);
				r.tm_dimer = enumerate_parallel<false>(e, w.par, w.rowmask, e.qlen, true, r.status);
				lap(t_enum);
			}
		}
		else{                                                                        // 1: heterodimer q x t; 2: the homodimer half of an oligo job (run_thermo_jobs splits those)
			const bool homo = (jb.mode == 2);
			const int TL = homo ? e.qlen : e.tlen;
			const int mxs = e.fill_wave(e.q, e.qlen, homo ? e.q : e.t, e.qlen, TL, 0);
			wave_sync();
			lap(t_fill);
			collect_rows(e, e.qlen, TL, 0, mxs, w.rowmask);
			wave_sync();
			lap(t_collect);
			r.tm_dimer = enumerate_parallel<false>(e, w.par, w.rowmask, e.qlen, homo, r.status);
			lap(t_enum);
		}
		if(lead){
			if(!V.map) out[j] = r;
			else if(r.status & 1u) V.word_bad[rec] = 2u;
			else if(r.tm_pm < V.tm_min || r.tm_pm > V.tm_max || r.tm_hairpin > V.max_hairpin) atomicOr(&V.word_bad[rec], 1u);   // valid_pcr.cpp:19-31
		}
		wave_sync();                                                                 // before the next job overwrites the sequences
		lap(t_other);
	}
	if(dbg_cycles && lead){
		atomicAdd(&dbg_cycles[0], t_fill); atomicAdd(&dbg_cycles[1], t_collect); atomicAdd(&dbg_cycles[2], t_enum); atomicAdd(&dbg_cycles[3], t_other);
	}
}

} // namespace thermo
