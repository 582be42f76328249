// The match scan, third form: the TARGETS are indexed, not scanned (included by pcr_device.hip after pcr_scan_seed2.inc).
//
// k_seed2 asks, for every one of a pass's ~1e8 target positions, whether the 9-gram there is one of the pass's ~6 000 seed codes:
// one LDS table probe per position, which is what bounds it (DESIGN.md section 4).  But where a 9-gram occurs in the targets does
// not depend on the pass: a counting sort of the set's positions by the 9-gram that starts there -- pix_first / pix_last[code] bound
// the run pix_ent[] of entries holding GLOBAL base positions (block * 32 + base; built once per load: EOS splits only invalidate windows, which the
// validity bits say) -- turns the question round: a seed (code, slot offset, orientation) is met at exactly the positions of its
// code's run, 1e8 / 2^18 = 380 of them on random sequence, and each implies ONE window (start = position - offset) to count
// exactly.  A pass then touches seeds x 380 = 2.2e6 windows instead of 1e8 positions, the same ~2-3e6 exact counts k_seed2 makes
// after its filter, and nothing else.
//
// Work: a CHUNK is 64 consecutive entries of one seed's run (a wave: one entry per lane, the seed's offset / orientation / mask
// entry uniform).  The host keeps a copy of the run lengths and lists, per pass, the running number of chunks per seed (per oligo
// the chunk counts are cached beside its seeds), deals the chunks to the launch's workgroups in equal contiguous shares and tells
// every workgroup -- by value, in the kernel arguments -- at which seed its share starts: a workgroup stages that slice of the list
// (some tens of entries), its waves take 8 chunks each, find their seeds by binary search in the slice (a lane each) and issue the
// 8 coalesced run reads (16 bytes per entry) back to back.  A window that reaches its orientation's floor (a fraction of a
// percent) goes on to the checks the tile form makes per tile or per window: validity bit (inside its sequence, no EOS,
// degeneracy), not in a tile the bit-sliced scan owns (IUPAC codes), active sequence -- the last two out of the block's info word --
// and is recorded exactly as s2_record does.  Every wave walks this chain of dependent loads once: the kernel is bound by its
// latency, not by bytes or instructions (DESIGN.md section 4 has the versions and what each removed).
// The irregular words come in through their own inverse index (pcr_scan_seed2.inc), a seed per lane, by the launch's first few
// workgroups (n_irr_wg), which read no chunks: that chain of dependent loads runs beside the chunk waves' instead of behind it.

constexpr uint32_t PIX_CODES = 1u << 18;
// The runs are sorted once more, by the base BEHIND the 9-gram: the sort key is 9-gram << 2 | code of base p + 9, so a 9-gram's run is four
// sub-runs side by side and pix_first / pix_last have PIX_KEYS entries.  A seed carries a span lo..hi of next bases (host: the 10-gram
// seeds of an oligo folded back into 9-gram seeds, pcr_host.hpp) and reads pix_first[code << 2 | lo] ... pix_last[code << 2 | hi]: a
// quarter of the run where the tenth base is fixed, all of it (lo..hi = A..T) where it is free.  The last 9-gram of a sequence is
// sorted under whatever tb holds behind it: a seed that constrains that base has offset <= 22, so its window covers p + 9 and
// leaves the sequence -- the validity bit says so.
constexpr uint32_t PIX_KEYS = PIX_CODES << 2;
constexpr uint32_t S3_BATCH = 8;

// a block of 32 positions: the 9-gram that starts at each (inside its sequence) -- counted, then scattered to its code's run together
// with the position's CONTEXT.  Every window a seed at p can imply (start p - offset, offset 0 ... 23, 32 bases) lies inside bases
// p - 23 ... p + 31, and the nine in the middle are the run's key: an entry is 16 bytes -- the position and the 2-bit codes of the 23
// bases on either side (92 bits) -- so a pass reads its runs in sequence, one 16-byte load per lane, and never gathers from the targets
// (a gather per window -- 2.2e6 random 128-byte lines per C2 pass -- made this form slower than the scan it replaces: 65 against 50 us).
template<bool SCATTER>
__global__ void k_pix_build(const uint32_t *__restrict__ tb, const uint32_t *__restrict__ blk_seq, const uint64_t *__restrict__ blk_off,
	const uint64_t *__restrict__ len, uint64_t total_blocks, uint32_t *__restrict__ count_or_cursor, uint4 *__restrict__ ent)
{
	const uint64_t b = (uint64_t)blockIdx.x*blockDim.x + threadIdx.x;
	if(b >= total_blocks) return;
	const uint32_t seq = blk_seq[b];
	const int64_t p0 = (int64_t)(b - blk_off[seq])*32, L = (int64_t)len[seq];
	uint32_t w[8];                                                               // tb words 2b - 2 ... 2b + 5: bases 32b - 32 ... 32b + 95 (tb is padded on both sides)
#pragma unroll
	for(int k = 0;k < 8;++k) w[k] = tb[(int64_t)2*(int64_t)b - 2 + k];
#pragma unroll
	for(int i = 0;i < 32;++i){
		if(p0 + i + 9 > L) break;
		const uint32_t ten = (i < 16) ? funnel(w[2], w[3], 2*i) : funnel(w[3], w[4], 2*(i - 16));   // bases p ... p + 15
		const uint32_t code = ((ten & S2_CODE_MASK) << 2) | ((ten >> 18) & 3u);                     // 9-gram << 2 | base p + 9
		if(SCATTER){
			const uint32_t at = atomicAdd(&count_or_cursor[code], 1u);
			// left = bases p - 23 ... p - 1, right = bases p + 9 ... p + 31 (46 bits each; the 9-gram between them is the run's key)
			const int jl = (i + 9) >> 4, sl = 2*((i + 9) & 15);                    // base p - 23 = base 32b - 32 + (i + 9)
			const int jr = (i + 41) >> 4, sr = 2*((i + 41) & 15);                  // base p + 9
			const uint32_t l_lo = funnel(w[jl], w[jl + 1], sl), l_hi = funnel(w[jl + 1], w[jl + 2], sl) & 0x3FFFu;
			const uint32_t r_lo = funnel(w[jr], w[jr + 1], sr), r_hi = funnel(w[jr + 1], w[jr + 2], sr) & 0x3FFFu;
			ent[at] = make_uint4((uint32_t)(b*32 + (uint64_t)i), l_lo, l_hi | (r_lo << 14), (r_lo >> 18) | (r_hi << 14));
		}
		else atomicAdd(&count_or_cursor[code], 1u);
	}
}

struct Seed3Tables {
	const uint32_t *seeds;        // as Seed2Tables
	const uint32_t *chunk_prefix; // [n_seeds + 1]: 64-entry chunks of the runs of the seeds before this one (host, per pass, from its copy of the run lengths)
	const uint8_t *spans;         // [n_seeds]: lo | hi << 2, the next bases (sub-runs of the code's run) the seed reads
	const uint4 *masks; const uint8_t *floors;
	uint32_t n_seeds, n_or, or_base;
	const uint32_t *pix_first, *pix_last; const uint4 *pix_ent;     // [PIX_KEYS] sub-run bounds; entry: position | left 23 bases, right 23 bases of its 9-gram (92 bits)
	uint32_t n_chunks, per_wg, slice_cap;   // workgroup w takes chunks [w * per_wg, (w + 1) * per_wg); LDS holds slice_cap list entries
	uint32_t n_irr_wg;                      // the launch's first n_irr_wg workgroups look the irregular words up and do nothing else (0: the chunk waves do it afterwards)
};
// Which seeds a workgroup's chunks belong to: start[w] = the last seed s with chunk_prefix[s] <= w * per_wg (host, a merge walk over the
// list), so workgroup w needs list entries start[w] ... start[w + 1] + 1 only -- some tens instead of the launch's thousands.  By value
// in the kernel arguments: there when the first instruction runs, no memory round trip of its own.
constexpr uint32_t S3_MAX_WG = 512;
constexpr uint32_t S3_MAX_OR = 448, S3_MAX_SEEDS = 1u << 16;   // orientations (9-bit ids, masks in LDS) and seeds of one launch of the third form
struct Seed3Slices { uint32_t start[S3_MAX_WG + 1]; };
struct Seed3Set {               // what the rare path reads of the sequence set: validity bits; per 32-base block its sequence (bit 31: the block's
	const uint32_t *valid, *blk_info, *blk_local; const uint8_t *active;   // tile holds IUPAC codes; bit 30: the sequence is not active -- kept in step
};                              // with active[] by k_blk_active, so that a survivor needs no round trip of its own for it) and its number within the sequence
constexpr uint32_t BLK_SEQ_MASK = 0x3FFFFFFFu, BLK_INACTIVE = 0x40000000u, BLK_DEGEN = 0x80000000u;

// The per-block words of a set, made where the set is: sequence (+ "its tile holds IUPAC codes", + "not active") and the block's
// number within its sequence.  tile0[q] = the first tile of sequence q in the set's tile arrays (host, n + 1 words).
__global__ void k_blk_info(const uint32_t *__restrict__ blk_seq, const uint64_t *__restrict__ blk_off, const uint64_t *__restrict__ len,
	const uint32_t *__restrict__ tile0, const uint8_t *__restrict__ tile_degen, const uint8_t *__restrict__ active, uint64_t total_blocks,
	uint32_t *__restrict__ blk_info, uint32_t *__restrict__ blk_local)
{
	const uint64_t b = (uint64_t)blockIdx.x*blockDim.x + threadIdx.x;
	if(b >= total_blocks) return;
	const uint32_t q = blk_seq[b];
	const uint64_t bl = b - blk_off[q], tile = bl >> 5;                            // 1 024 window starts per tile = 32 blocks
	const uint32_t nt = tile0[q + 1] - tile0[q];
	const bool degen = tile < nt && tile_degen[tile0[q] + tile];
	blk_info[b] = q | (degen ? 0x80000000u : 0u) | (active[q] ? 0u : 0x40000000u);
	blk_local[b] = (uint32_t)bl;
}

__global__ void k_blk_active(uint32_t *__restrict__ blk_info, const uint32_t *__restrict__ blk_seq, const uint8_t *__restrict__ active, uint64_t total_blocks)
{
	const uint64_t b = (uint64_t)blockIdx.x*blockDim.x + threadIdx.x;
	if(b >= total_blocks) return;
	const uint32_t v = blk_info[b] & ~BLK_INACTIVE;
	blk_info[b] = v | (active[blk_seq[b]] ? 0u : BLK_INACTIVE);
}

// The irregular words through their inverse index: 16 of the launch's seeds per wave turn (a lane each fetches its key's run),
// the runs' entries dealt to the 64 lanes (entry t belongs to the lane whose inclusive count first exceeds t): word -> record ->
// live (size counter, active sequence) -> exact slot count.  gw / n_gw: this wave's number among the waves that share the seeds.
__device__ __forceinline__ void s3_irregular(const Seed3Tables &T3, const Seed3Set &Q, const IrrArgs2 &IA, const uint4 *__restrict__ cand_fwd,
	const uint32_t *__restrict__ cand_floor, HitSink sink, uint32_t gw, uint32_t n_gw, uint32_t lane)
{
	for(uint32_t i0 = gw*16u;i0 < T3.n_seeds;i0 += n_gw*16u){                   // (uniform per wave)
		const uint32_t i = i0 + lane;
		const uint32_t sdv = (lane < 16u && i < T3.n_seeds) ? T3.seeds[i] : S2_END;
		const uint32_t orient = T3.or_base + (sdv & 0x1FFu);
		uint32_t first = 0, cnt = 0;
		if(sdv != S2_END && !(orient & 1u)){                                     // forward orientations only (as the scan of the words does)
			const uint32_t key = (((sdv >> 9) & 31u) << 18) | (sdv >> 14);
			first = IA.ix_first[key]; cnt = IA.ix_last[key] - first;
		}
		const uint32_t incl = s2_scan(cnt);
		const uint32_t total = s2_rl(incl, 63);
		for(uint32_t t0 = 0;t0 < total;t0 += 64u){
			const uint32_t t = t0 + lane;
			uint32_t lo = 0;                                                      // the first lane whose inclusive count exceeds t: six halvings
#pragma unroll
			for(uint32_t stp = 32u;stp;stp >>= 1){ if((uint32_t)__shfl((int)incl, (int)(lo + stp - 1u)) <= t) lo += stp; }
			const int sl = (int)min(lo, 63u);
			const uint32_t s_incl = (uint32_t)__shfl((int)incl, sl), s_cnt = (uint32_t)__shfl((int)cnt, sl), s_first = (uint32_t)__shfl((int)first, sl);
			const uint32_t c = (uint32_t)__shfl((int)orient, sl) >> 1;
			if(t >= total) continue;
			const IrrDev e = IA.irr[IA.ix_words[s_first + (t - (s_incl - s_cnt))]];
			if(((e.meta >> 8) & 0xFFu) < IA.min_cws || !Q.active[e.seq]) continue;
			const uint32_t n = match_count(e.w.a, e.w.c, e.w.g, e.w.t, cand_fwd[c]);
			if(n >= cand_floor[c]) record_hit(sink, e.seq, c, make_key(e.seq, e.loc, e.meta & 0xFF, 1, (e.meta >> 16) & 0xFF), n);
		}
	}
}

template<uint32_t S3_THREADS>
__global__ __launch_bounds__(S3_THREADS) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_seed3(Seed3Tables T3, Seed3Set Q, IrrArgs2 IA, const uint4 *__restrict__ cand_fwd, const uint32_t *__restrict__ cand_floor,
	HitSink sink, S2Clear Z, Seed3Slices W)
{
#include "pcr_scan_seed3_pass.inc"
}

// Two passes of different handles in one launch: row blockIdx.y runs its pass on half the workgroups (gridDim.x = half of k_seed3's
// grid) with twice the share of chunks each.  The rows share nothing -- each has its own tables, set, sink and regions to clear --
// so there is no order between them inside the launch; the dynamic LDS is the larger of the two needs.  Two full Seed3Slices would
// not fit the kernel-argument segment: a row's slices are every second entry of its pass's plan (the host derives them).
struct Seed3Row {
	Seed3Tables T3; Seed3Set Q; IrrArgs2 IA; const uint4 *cand_fwd; const uint32_t *cand_floor; HitSink sink; S2Clear Z;
};
struct Seed3HalfSlices { uint32_t start[S3_MAX_WG/2 + 1]; };
template<uint32_t S3_THREADS>
__global__ __launch_bounds__(S3_THREADS) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_seed3_pair(Seed3Row A, Seed3HalfSlices WA, Seed3Row B, Seed3HalfSlices WB)
{
	// (a uniform branch and references into the kernel's own arguments: a row's arguments stay in scalar registers and in the
	// kernel-argument segment; a dynamically indexed copy of the rows would go to scratch whole)
	if(blockIdx.y == 0){
		const Seed3Tables &T3 = A.T3; const Seed3Set &Q = A.Q; const IrrArgs2 &IA = A.IA; const uint4 *const cand_fwd = A.cand_fwd; const uint32_t *const cand_floor = A.cand_floor;
		const HitSink &sink = A.sink; const S2Clear &Z = A.Z; const Seed3HalfSlices &W = WA;
#include "pcr_scan_seed3_pass.inc"
	}
	else{
		const Seed3Tables &T3 = B.T3; const Seed3Set &Q = B.Q; const IrrArgs2 &IA = B.IA; const uint4 *const cand_fwd = B.cand_fwd; const uint32_t *const cand_floor = B.cand_floor;
		const HitSink &sink = B.sink; const S2Clear &Z = B.Z; const Seed3HalfSlices &W = WB;
#include "pcr_scan_seed3_pass.inc"
	}
}
