// v2 match scan (included by pcr_device.hip): bit-sliced over candidate orientations.
//
// One lane = one window start p.  Bit j of a 32-bit register = candidate orientation j of the
// current group (orientation = 2*candidate + {0: masks as stored, 1: reverse-complemented}).
// For every slot k the lane looks up, in an LDS table indexed by the TARGET nibble at p+k, the
// word "which orientations accept this base set at slot k" and adds it into a bit-sliced
// counter with carry-save adders (v_bitop3_b32: xor3 + majority = 2 ops per adder).  The counter
// starts at (32 - floor_j), so "count_j >= floor_j" is "a carry left bit 4", collected in `hi`.
// Only lanes with a non-zero `hi` (rare) take the exact slow path (plane popcount + record_hit).
//
// Work per (position, 32 orientations): ~2.2 VALU ops per slot, against 6 per single
// (position, orientation) in the v1 kernel.  No IUPAC case is special: the table row is indexed
// by the 4-bit target code, the table bits come from the 4-bit oligo code.

template<int NW> struct WVec { uint32_t v[NW]; };

template<int NW> struct ScanState {
	WVec<NW> run[5];    // bit-sliced counter planes: ones, twos, fours, eights, sixteens
	WVec<NW> pend[5];   // pending carry per level (index 1..4 used)
	WVec<NW> hi;        // OR of carries out of the sixteens plane
};

template<int NW>
__device__ __forceinline__ void csa(WVec<NW> &run, const WVec<NW> &a, const WVec<NW> &b, WVec<NW> &carry)
{
#pragma unroll
	for(int w = 0;w < NW;++w){
		const uint32_t r = run.v[w];
		carry.v[w] = __builtin_amdgcn_bitop3_b32(r, a.v[w], b.v[w], 0xE8);   // majority
		run.v[w] = __builtin_amdgcn_bitop3_b32(r, a.v[w], b.v[w], 0x96);     // xor3
	}
}

template<int NW>
__device__ __forceinline__ void half_add(WVec<NW> &run, const WVec<NW> &a, WVec<NW> &carry)
{
#pragma unroll
	for(int w = 0;w < NW;++w){
		const uint32_t r = run.v[w];
		carry.v[w] = r & a.v[w];
		run.v[w] = r ^ a.v[w];
	}
}

constexpr int trailing_ones(int j) { int t = 0; while(j & 1){ ++t; j >>= 1; } return t; }

// Add the J-th pair of one-bit inputs (binary-counter schedule: level l holds a pending carry
// iff bit l-1 of J is set).
template<int NW, int J>
__device__ __forceinline__ void pair_step(ScanState<NW> &s, const WVec<NW> &x0, const WVec<NW> &x1)
{
	WVec<NW> carry, c2;
	csa<NW>(s.run[0], x0, x1, carry);
	constexpr int t = trailing_ones(J);
	if constexpr (t >= 1){ csa<NW>(s.run[1], s.pend[1], carry, c2); carry = c2; }
	if constexpr (t >= 2){ csa<NW>(s.run[2], s.pend[2], carry, c2); carry = c2; }
	if constexpr (t >= 3){ csa<NW>(s.run[3], s.pend[3], carry, c2); carry = c2; }
	if constexpr (t >= 4){ csa<NW>(s.run[4], s.pend[4], carry, c2); carry = c2; }
	if constexpr (t + 1 <= 4){ s.pend[t + 1] = carry; }
	else{
#pragma unroll
		for(int w = 0;w < NW;++w) s.hi.v[w] |= carry.v[w];
	}
}

// After NPAIR pairs: fold the still-pending carries (the set bits of NPAIR) upwards.
template<int NW, int NPAIR>
__device__ __forceinline__ void flush_pending(ScanState<NW> &s)
{
	WVec<NW> carry, c2;
	bool have = false;
#pragma unroll
	for(int l = 1;l <= 4;++l){
		const bool pend = ((NPAIR >> (l - 1)) & 1) != 0;
		if(pend && have){ csa<NW>(s.run[l], s.pend[l], carry, c2); carry = c2; have = true; }
		else if(pend){ half_add<NW>(s.run[l], s.pend[l], carry); have = true; }
		else if(have){ half_add<NW>(s.run[l], carry, c2); carry = c2; have = true; }
	}
	if(have){
#pragma unroll
		for(int w = 0;w < NW;++w) s.hi.v[w] |= carry.v[w];
	}
}

// LDS row of slot k' for the target nibble at window slot K (compile-time K).
template<int NW, int K>
__device__ __forceinline__ void fetch_row(const uint32_t *__restrict__ lds_tab, int kprime, const uint32_t (&n)[4], WVec<NW> &x)
{
	constexpr int sh = (K & 7)*4;
	const uint32_t word = n[K >> 3];
	uint32_t off;   // nibble * 32 bytes
	if constexpr (sh >= 5) off = (word >> (sh - 5)) & 0x1E0u;
	else off = (word << (5 - sh)) & 0x1E0u;
	const char *row = (const char *)lds_tab + kprime*512 + off;
	if constexpr (NW <= 4){
		const uint4 a = *(const uint4 *)row;
		const uint32_t t[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
		for(int w = 0;w < NW;++w) x.v[w] = t[w];
	}
	else{
		const uint4 a = *(const uint4 *)row;
		uint4 b = *(const uint4 *)(row + 16);
		// keep the second read a ds_read_b128 (4 LDS cycles): a 3-word ds_read_b96 costs 8
		if constexpr (NW == 7) asm volatile("" : "+v"(b.w));
		const uint32_t t[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
		for(int w = 0;w < NW;++w) x.v[w] = t[w];
	}
}

template<int NW, int KLO, int J, int NPAIR>
struct SlotLoop {
	static __device__ __forceinline__ void run(ScanState<NW> &s, const uint32_t *__restrict__ lds_tab, const uint32_t (&n)[4])
	{
		WVec<NW> x0, x1;
		fetch_row<NW, KLO + 2*J>(lds_tab, 2*J, n, x0);
		fetch_row<NW, KLO + 2*J + 1>(lds_tab, 2*J + 1, n, x1);
		pair_step<NW, J>(s, x0, x1);
		SlotLoop<NW, KLO, J + 1, NPAIR>::run(s, lds_tab, n);
	}
};
template<int NW, int KLO, int NPAIR>
struct SlotLoop<NW, KLO, NPAIR, NPAIR> {
	static __device__ __forceinline__ void run(ScanState<NW> &, const uint32_t *__restrict__, const uint32_t (&)[4]) {}
};

// Exact re-evaluation of the orientations flagged by the bit-sliced counter for window p
// (plane popcount, as the v1 kernel) and hit recording.  Out of line: it runs for <1 % of lanes.
// Its launch-constant arguments travel as ONE pointer to a copy in LDS: as thirteen register arguments plus the
// 48-byte HitSink they overflowed the register calling convention and gave every k_scan2 80 bytes of scratch per lane.
struct Scan2Slow {
	const uint32_t *orient_ids; const uint4 *planes; const uint32_t *valid;
	const uint4 *cand_fwd, *cand_rc; const uint32_t *cand_floor; uint32_t ncand; uint32_t pad;
	HitSink sink;
};

__device__ __noinline__ void scan2_slow_path(uint32_t bits, uint32_t o_base, uint32_t p, uint32_t seq, uint64_t base, const Scan2Slow *A)
{
	const uint32_t b = p >> 5, sh = p & 31;
	if(!((A->valid[base + b] >> sh) & 1u)) return;
	const uint4 lo = A->planes[base + b];
	const uint4 hi4 = A->planes[base + b + 1];
	const uint32_t wa = funnel(lo.x, hi4.x, sh), wc = funnel(lo.y, hi4.y, sh);
	const uint32_t wg = funnel(lo.z, hi4.z, sh), wt = funnel(lo.w, hi4.w, sh);
	const uint32_t *orient_ids = A->orient_ids;
	const uint32_t ncand = A->ncand;
	while(bits){
		const uint32_t j = __ffs(bits) - 1;
		bits &= bits - 1;
		const uint32_t o = orient_ids ? orient_ids[o_base + j] : o_base + j;   // bit -> orientation (2*candidate + rc)
		const uint32_t c = o >> 1;
		if(c >= ncand) continue;
		const uint32_t fl = A->cand_floor[c];
		if(o & 1){
			const uint32_t cnt = match_count(wa, wc, wg, wt, A->cand_rc[c]);
			if(cnt >= fl) record_hit_inline(A->sink, seq, c, make_key(seq, (int32_t)p + 31, 2, 0, 0), cnt);   // sequence.cpp:190 (inline: a call out of this out-of-line function needs a stack frame)
		}
		else{
			const uint32_t cnt = match_count(wa, wc, wg, wt, A->cand_fwd[c]);
			if(cnt >= fl) record_hit_inline(A->sink, seq, c, make_key(seq, (int32_t)p, 1, 0, 0), cnt);        // sequence.cpp:184
		}
	}
}

constexpr int SCAN2_THREADS = 256;
constexpr int SCAN2_NPOS = TILE_POS/SCAN2_THREADS;

// grid.x = tiles, grid.y = orientation groups of this launch (group index = group0 + blockIdx.y).
// tab : [group][NSLOT][16][8] u32     bias : [group][6][8] u32
template<int NW, int NSLOT, int KLO>
__global__ __launch_bounds__(SCAN2_THREADS) void k_scan2(
	const uint32_t *__restrict__ nib, const uint4 *__restrict__ planes, const uint32_t *__restrict__ valid,
	const uint64_t *__restrict__ blk_off, const uint64_t *__restrict__ len, const uint8_t *__restrict__ active,
	const uint32_t *__restrict__ tile_seq, const uint32_t *__restrict__ tile_pos0,
	const uint32_t *__restrict__ tab, const uint32_t *__restrict__ bias, uint32_t group0, uint32_t group_words /* counter words a group spans (Scan2Tables::gw) */,
	const uint32_t *__restrict__ tile_ids /* NULL = all tiles */, const uint32_t *__restrict__ orient_ids /* NULL = identity */,
	const uint4 *__restrict__ cand_fwd, const uint4 *__restrict__ cand_rc, const uint32_t *__restrict__ cand_floor,
	uint32_t ncand, HitSink sink)
{
	static_assert(NSLOT % 2 == 0 && KLO + NSLOT <= 32, "slot range");
	__shared__ __attribute__((aligned(16))) uint32_t lds_tab[NSLOT*16*8];
	__shared__ Scan2Slow slow_args;
	const uint32_t tile = tile_ids ? tile_ids[blockIdx.x] : blockIdx.x;
	const uint32_t seq = tile_seq[tile];
	if(!active[seq]) return;
	if(threadIdx.x == 0){
		slow_args.orient_ids = orient_ids; slow_args.planes = planes; slow_args.valid = valid; slow_args.cand_fwd = cand_fwd; slow_args.cand_rc = cand_rc;
		slow_args.cand_floor = cand_floor; slow_args.ncand = ncand; slow_args.pad = 0; slow_args.sink = sink;
	}
	const uint32_t group = group0 + blockIdx.y;
	{
		const uint4 *src = (const uint4 *)(tab + (size_t)group*(NSLOT*16*8));
		uint4 *dst = (uint4 *)lds_tab;
		for(int i = threadIdx.x;i < NSLOT*16*8/4;i += SCAN2_THREADS) dst[i] = src[i];
	}
	__syncthreads();
	const uint64_t L = len[seq];
	const uint64_t base = blk_off[seq];
	const uint32_t p0 = tile_pos0[tile];
	const uint32_t *bg = bias + (size_t)group*48;

#pragma unroll 1
	for(int i = 0;i < SCAN2_NPOS;++i){
		const uint32_t p = p0 + threadIdx.x + SCAN2_THREADS*i;
		if((uint64_t)p + 32 > L) continue;
		// 32-nibble window starting at p (nibble j of word w = base 8w+j)
		uint32_t n[4];
		{
			const uint32_t *src = nib + base*4 + (p >> 3);
			const uint32_t sh = (p & 7)*4;
			const uint32_t a0 = src[0], a1 = src[1], a2 = src[2], a3 = src[3], a4 = src[4];
			n[0] = funnel(a0, a1, sh); n[1] = funnel(a1, a2, sh); n[2] = funnel(a2, a3, sh); n[3] = funnel(a3, a4, sh);
		}
		ScanState<NW> s;
#pragma unroll
		for(int l = 0;l < 5;++l){
#pragma unroll
			for(int w = 0;w < NW;++w) s.run[l].v[w] = bg[l*8 + w];
		}
#pragma unroll
		for(int w = 0;w < NW;++w) s.hi.v[w] = bg[5*8 + w];
		SlotLoop<NW, KLO, 0, NSLOT/2>::run(s, lds_tab, n);
		flush_pending<NW, NSLOT/2>(s);

		// Rare path.  `s` must never be indexed dynamically (that would send the whole counter
		// state to scratch): every word is passed by value to an out-of-line helper.
		uint32_t any = 0;
#pragma unroll
		for(int w = 0;w < NW;++w) any |= s.hi.v[w];
		if(any){
#pragma unroll
			for(int w = 0;w < NW;++w){
				if(s.hi.v[w]) scan2_slow_path(s.hi.v[w], (group*group_words + w)*32, p, seq, base, &slow_args);
			}
		}
	}
}

// Host side: lookup tables + bias planes for all orientation groups.
struct Scan2Tables {
	int nslot, klo;
	uint32_t gw;             // counter words per group: 8 (256 orientations).  Groups of 4 words (50 VGPRs instead of 114 - 120, twice the waves, one
	                         // more pass over the positions) measured slower: 0.548 against 0.524 ms per select_words at C3 (7 words), 2.23 against 2.09 at 16
	uint32_t n_groups;       // groups of gw words
	uint32_t last_words;     // words used by the last group (1..gw)
	std::vector<uint32_t> tab, bias;
};

// `orients`: the orientations (2*candidate + rc) to put on the counter bits, in bit order.
inline void build_scan2_tables(const std::vector<pcrhost::Candidate> &cand, const std::vector<uint32_t> &orients, Scan2Tables &T)
{
	const uint32_t n_or = (uint32_t)orients.size();
	uint32_t occ = 0;
	for(uint32_t o : orients){ const pcrhost::Candidate &c = cand[o >> 1]; occ |= pcrhost::planes_occupied((o & 1) ? c.rc : c.fwd); }
	// slots 3..28 cover centred 18-25-mers in both orientations (pcr_assay.cpp:719)
	if((occ & ~0x1FFFFFF8u) == 0){ T.nslot = 26; T.klo = 3; }
	else{ T.nslot = 32; T.klo = 0; }
	const uint32_t n_words = (n_or + 31)/32;
	T.gw = 8;
	T.n_groups = (n_words + T.gw - 1)/T.gw;
	T.last_words = n_words - (T.n_groups - 1)*T.gw;
	T.tab.assign((size_t)T.n_groups*T.nslot*16*8, 0u);
	T.bias.assign((size_t)T.n_groups*48, 0u);
	for(uint32_t bit = 0;bit < n_or;++bit){
		const uint32_t o = orients[bit];
		const pcrhost::Candidate &c = cand[o >> 1];
		const Planes &m = (o & 1) ? c.rc : c.fwd;
		const uint32_t g = (bit >> 5)/T.gw, w = (bit >> 5) % T.gw, j = bit & 31;
		if(c.floor_ > 32) continue;   // can never be reached: leave the orientation dead
		const uint32_t b = 32 - c.floor_;
		for(int l = 0;l < 6;++l){ if((b >> l) & 1) T.bias[(size_t)g*48 + l*8 + w] |= (1u << j); }
		for(int kp = 0;kp < T.nslot;++kp){
			const unsigned code = pcrhost::planes_nibble(m, T.klo + kp);
			if(!code) continue;
			for(unsigned tb = 1;tb < 16;++tb){
				if(code & tb) T.tab[(((size_t)g*T.nslot + kp)*16 + tb)*8 + w] |= (1u << j);
			}
		}
	}
}
