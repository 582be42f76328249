// MI355X (gfx950) implementation of the C-ABI in include/pcramp_hip.h.
//
// HBM layout (per sequence set)
//   planes[]  : one uint4 {A,C,G,T} per 32-base block; bit j of .x = base 32*b+j may be 'A', ...
//               (the reference's 4-bit IUPAC nibble, bit-transposed: same 4 bits/base as
//               Sequence::seq_buffer, sequence.h:86).  EOS / past-the-end = no bit in any plane.
//               Each sequence owns ceil(L/32)+2 blocks (two zero halo blocks).
//   nib[]     : the same codes as 4 u32 per block, nibble j%8 of word j/8 = base 32*b+j (table index of
//               the bit-sliced scan, pcr_scan_bitsliced.inc).
//   tb[]      : 2 bits per base (A,C,G,T = 0..3, anything else 0), 2 u32 per block: q-gram codes of the seed scan.
//   valid[]   : one u32 per block; bit j = the 32-base window starting at 32*b+j is a REGULAR
//               window that Sequence::pack emits (sequence.cpp:127-153 filters applied).
//   irr[]     : explicit irregular words (pcr_host.hpp); irr_scan[]: the same in scan order as 2-bit codes (k_seed2).
//   tile_desc[]: one 16-byte descriptor per 1024-window tile (k_seed2).
// Kernels
//   k_transpose, k_valid, k_tile_degen, k_tile_desc : load-time index build (replaces Sequence::operator= + the filter half of pack)
//   k_stage                : per-pass tables out of host-mapped memory + clearing of the pass's control block
//   k_seed2                : the default match scan: seed filter on 9-grams, tables built in LDS (pcr_scan_seed2.inc)
//   k_seed (+ k_seed_tables, scan_irr_block), k_scan2, k_scan, k_scan_irr :
//                            the other forms of the oligo x window match scan + per-(sequence,candidate) running max
//                            (select_words.cpp:88-117 over the implicit word index); pcr_scan_seed.inc,
//                            pcr_scan_bitsliced.inc
//   k_touched, k_finalize, k_post : per-sequence arg-max-with-ties filter, sort, dedupe -> the device word DB
//                            (select_words.cpp:100-138); k_post = the whole tail of the fused pass in one launch
//   k_match, k_pair        : match_words / find_oligo_match / find_amplicon_match / update_identity /
//                            sqrtf(f*r) test (optimize.cpp:209-301, pcr_assay.cpp:12-69,338-441,544-578)
//   k_pair_moves, k_pair_moves_batch : the same sweep for the trial words of a local-search move (optimize_pcr.cpp; pcr_optimize.inc)
//   k_sw, k_sw_words, k_bg_*, k_mx_* : SeqOverlap Smith-Waterman and the background / multiplex screens (pcr_sw.inc)
//   thermo::k_thermo_wave  : NucCruc (pcr_thermo.inc)
//   k_site_tm, k_site_reduce : the same engine over the binding sites of the word DB, jobs built on the device (pcr_site_tm.inc)
//   k_sv_items, k_sv_heads, k_sv_tm : the sites grouped by (oligo, template planes in the window) with radix sorts over the whole key, one melt per group (pcr_site_variants.inc)
//   k_rp_candidates, k_rp_weigh, k_rp_step : a greedy union of variants into each oligo, every (oligo, candidate) weighed by what its union holds (pcr_site_repair.inc)
//   k_pool_dimer, k_pool_dimer_reduce : the same engine over every ordered oligo pair of a pool, jobs derived from the job number (pcr_pool_dimers.inc)
//   k_dimer_end3_scan, k_dimer_end3_melt, k_dimer_end3_merge : the 3'-anchored placements of those pairs, listed from the slot masks and melted run by run (pcr_pool_dimers_end3.inc)
//   k_item_tm, k_products_join : k_site_tm's Tm per item, and k_pool_join's geometry with the two sites' Tm, the floor and the pool's bit rows (pcr_products_tm.inc)
//   k_item_end3, k_end3_join : the 3' end of every item's site (clamp, mismatches in a window, identity with the TaqMAMA factor), and k_products_join with a rule on the two sites' ends (pcr_products_end3.inc)
//   k_anneal_join, k_anneal_rows : the same join without a floor: per (pool pair, sequence) the highest min-Tm by integer atomicMax, LDS histograms over an ascending temperature list (pcr_anneal_profile.inc)
//   k_probe_products, k_probe_hits : the kept products of the primers compacted, then a wave per product over the probe items inside it (pcr_probe_hits.inc)
//   k_amp_scan, k_amp_verify, k_amp_extract : eight lanes per product record over its bases: G+C, a hash of its spelling, equality with its group's first, the packed text (pcr_pool_amplicons.inc)
// Host side in the same library: pcr_optimize.inc (optimize() batched over trial assays), pcr_sampler.inc, pcr_multiplex.inc,
// pcr_multiplex_screen.inc, pcr_writers.inc; pcr_exchange.inc: the bitset all-gather over RCCL.
#include <hip/hip_runtime.h>
#include <cstring>
#include <rocprim/device/device_radix_sort.hpp>

#include <stdint.h>
#include <string.h>
#include <math.h>
#include <stdlib.h>
#include <string>
#include <vector>
#include <chrono>
#include <algorithm>
#include <unordered_map>
#include <type_traits>
#include <thread>
#include <mutex>
#include <condition_variable>
#include <functional>
#include <memory>
#include <atomic>
#include <cassert>
#include <sched.h>
#include <pthread.h>

#include "../../include/pcramp_hip.h"
#include "pcr_host.hpp"
#include "pcr_seed_lists.hpp"
#include "pcr_launch_queue.hpp"

using pcrhost::Planes;

namespace { thread_local std::string g_err; }
#include "pcr_owned.hpp"

namespace {

using pcrown::DevBuf; using pcrown::MappedBuf; using pcrown::Event; using pcrown::Stream;

#define HIP_TRY(expr) do{ hipError_t e_ = (expr); if(e_ != hipSuccess){ \
	g_err = std::string(#expr) + ": " + hipGetErrorString(e_); return PCR_ERR_DEVICE; } }while(0)

constexpr int TILE_POS = 1024;       // window starts per workgroup
constexpr int SCAN_THREADS = 256;
constexpr int SCAN_NPOS = TILE_POS/SCAN_THREADS;

// dedupe / sort key of a DB entry: [seq:24][loc+64:32][strand-1:1][kind:1][ord:6]
constexpr int KEY_SEQ_SHIFT = 40;
constexpr int KEY_LOC_SHIFT = 8;
constexpr int LOC_BIAS = 64;

struct Hit { uint64_t key; uint32_t cand; uint32_t cnt; };

// host-mapped mailbox slot: a pass's counters, then its sequence number (release store)
struct PassMail { volatile uint32_t counters[4]; volatile uint32_t seq; uint32_t pad[11]; };

constexpr uint32_t N_TOUCHED_UNKNOWN_DEV = 0xFFFFFFFFu;   // published instead of a touched count by the fused tail

struct IrrDev { Planes w; int32_t loc; uint32_t seq; uint32_t meta; /* strand | cws<<8 | ord<<16 */ uint32_t local_id; };

struct DevEntry { Planes w; int32_t loc; uint32_t seq; uint32_t strand; uint32_t pad; };

struct OligoDev {        // one assay oligo for the amplicon screen
	Planes m;
	uint32_t floor2;     // unsigned(size * thr^2), optimize.cpp:293
	float norm;          // float(1.0/len), optimize.cpp:221
	int32_t start, stop; // Word::start()/stop()
	uint32_t p1, p2;     // last two primer bases (optimize.cpp:236)
};

__constant__ float c_taq_mama[256];

// word.cpp:252-272 -- Table 2 of Li et al., Genomics 83 (2004) 311-320 (rows: template pair,
// columns: primer pair, order {CC,GC,AC,TC,CG,GG,AG,TG,CA,GA,AA,TA,CT,GT,AT,TT}).
const float h_taq_mama[256] = {
	1.000f, 0.968f, 0.947f, 1.034f, 0.547f, 0.253f, 0.230f, 0.359f, 0.606f, 0.282f, 0.372f, 0.347f, 0.957f, 0.382f, 0.399f, 0.687f,
	0.989f, 1.000f, 1.023f, 1.000f, 0.420f, 0.662f, 0.445f, 0.367f, 0.870f, 0.512f, 0.492f, 0.508f, 0.372f, 1.000f, 0.492f, 0.714f,
	1.011f, 1.000f, 1.000f, 1.000f, 0.459f, 0.277f, 0.570f, 0.343f, 0.927f, 0.362f, 0.590f, 0.542f, 0.439f, 0.488f, 0.978f, 0.662f,
	1.000f, 0.907f, 1.000f, 1.000f, 0.382f, 0.234f, 0.228f, 0.542f, 0.763f, 0.309f, 0.410f, 0.473f, 0.426f, 0.347f, 0.423f, 0.947f,
	0.590f, 0.334f, 0.445f, 0.323f, 1.000f, 0.978f, 0.927f, 0.989f, 0.907f, 0.645f, 0.525f, 0.455f, 0.927f, 0.408f, 0.408f, 0.707f,
	0.327f, 0.595f, 0.319f, 0.396f, 0.947f, 1.000f, 0.978f, 0.989f, 0.405f, 0.861f, 0.681f, 0.512f, 0.410f, 0.968f, 0.452f, 0.714f,
	0.410f, 0.420f, 0.590f, 0.311f, 1.023f, 1.000f, 1.000f, 1.000f, 0.488f, 0.898f, 0.907f, 0.566f, 0.442f, 0.449f, 0.989f, 0.707f,
	0.423f, 0.343f, 0.305f, 0.585f, 1.034f, 0.879f, 0.927f, 1.000f, 0.473f, 0.720f, 0.547f, 0.957f, 0.459f, 0.374f, 0.459f, 1.023f,
	1.023f, 0.429f, 0.473f, 0.477f, 1.023f, 0.466f, 0.420f, 0.477f, 1.000f, 0.978f, 0.907f, 0.978f, 0.907f, 0.380f, 0.525f, 0.669f,
	0.442f, 1.046f, 0.455f, 0.470f, 0.432f, 1.058f, 0.481f, 0.485f, 0.917f, 1.000f, 1.023f, 1.023f, 0.336f, 0.968f, 0.534f, 0.639f,
	0.617f, 0.452f, 1.011f, 0.439f, 0.492f, 0.504f, 0.978f, 0.462f, 0.989f, 0.947f, 1.000f, 0.978f, 0.405f, 0.405f, 0.888f, 0.606f,
	0.601f, 0.377f, 0.377f, 1.046f, 0.500f, 0.399f, 0.408f, 1.034f, 0.978f, 0.720f, 0.870f, 1.000f, 0.402f, 0.313f, 0.651f, 0.927f,
	0.978f, 0.462f, 0.466f, 0.488f, 0.420f, 0.239f, 0.225f, 0.336f, 0.504f, 0.269f, 0.319f, 0.656f, 1.000f, 0.835f, 0.907f, 1.034f,
	0.429f, 1.011f, 0.473f, 0.477f, 0.340f, 0.413f, 0.357f, 0.354f, 0.352f, 0.538f, 0.413f, 0.794f, 0.927f, 1.000f, 1.058f, 1.000f,
	0.595f, 0.492f, 0.968f, 0.485f, 0.367f, 0.282f, 0.388f, 0.439f, 0.413f, 0.309f, 0.566f, 0.917f, 0.957f, 0.957f, 1.000f, 0.989f,
	0.590f, 0.380f, 0.410f, 0.968f, 0.364f, 0.223f, 0.230f, 0.416f, 0.321f, 0.239f, 0.301f, 0.645f, 0.978f, 0.714f, 0.947f, 1.000f
};

// ============================================================================== device helpers
__device__ __forceinline__ uint32_t funnel(uint32_t lo, uint32_t hi, uint32_t sh)
{
	return __builtin_amdgcn_alignbit(hi, lo, sh);   // ({hi,lo} >> (sh & 31)) & 0xffffffff
}

__device__ __forceinline__ uint32_t match_count(uint32_t wa, uint32_t wc, uint32_t wg, uint32_t wt, const uint4 m)
{
	// # slots whose base sets intersect == Word::operator& (word.cpp:151-154) in plane form
	return __popc((wa & m.x) | (wc & m.y) | (wg & m.z) | (wt & m.w));
}

// ============================================================================== load-time kernels
// One thread per 32-base block: nibbles (high first, sequence.h:223-228) -> four bit planes.
__global__ void k_transpose(const uint8_t *__restrict__ packed, const uint64_t *__restrict__ byte_off,
	const uint64_t *__restrict__ len, const uint64_t *__restrict__ blk_off, const uint32_t *__restrict__ blk_seq,
	uint4 *__restrict__ planes, uint32_t *__restrict__ nib, uint32_t *__restrict__ tb, uint64_t total_blocks)
{
	const uint64_t gb = (uint64_t)blockIdx.x*blockDim.x + threadIdx.x;
	if(gb >= total_blocks) return;
	const uint32_t s = blk_seq[gb];
	const uint64_t b = gb - blk_off[s];
	const uint64_t L = len[s];
	const uint8_t *src = packed + byte_off[s];
	uint32_t a = 0, c = 0, g = 0, t = 0;
	uint32_t nw[4] = {0, 0, 0, 0};   // the same 32 codes, nibble j%8 of word j/8 (v2 scan's table index)
	uint32_t tw[2] = {0, 0};
	for(int j = 0;j < 32;++j){
		const uint64_t pos = b*32 + j;
		if(pos >= L) break;
		const uint8_t v = src[pos >> 1];
		const uint32_t code = (pos & 1) ? (v & 0xF) : (v >> 4);
		a |= (code & 1u) << j;
		c |= ((code >> 1) & 1u) << j;
		g |= ((code >> 2) & 1u) << j;
		t |= ((code >> 3) & 1u) << j;
		nw[j >> 3] |= code << ((j & 7)*4);
		// 2-bit code for the seed scan: A,C,G,T -> 0..3; anything else (IUPAC, EOS) -> 0
		const uint32_t c2 = (code == 2) ? 1u : (code == 4) ? 2u : (code == 8) ? 3u : 0u;
		tw[j >> 4] |= c2 << ((j & 15)*2);
	}
	planes[gb] = make_uint4(a, c, g, t);
	((uint4 *)nib)[gb] = make_uint4(nw[0], nw[1], nw[2], nw[3]);
	((uint2 *)tb)[gb] = make_uint2(tw[0], tw[1]);
}

// One thread per block: validity of the 32 windows that START in it.  A window is regular iff
// all 32 slots are non-EOS; then pack's filters (GC first, then degeneracy; sequence.cpp:127-153).
__global__ void k_valid(const uint4 *__restrict__ planes, const uint64_t *__restrict__ blk_off,
	const uint32_t *__restrict__ blk_seq, const uint64_t *__restrict__ nblk_real, uint32_t *__restrict__ valid,
	uint64_t total_blocks, uint32_t max_degen, uint64_t gc_ok, uint64_t first_block, uint64_t n_blocks)
{
	const uint64_t i = (uint64_t)blockIdx.x*blockDim.x + threadIdx.x;
	if(i >= n_blocks) return;
	const uint64_t gb = first_block + i;
	if(gb >= total_blocks) return;
	const uint32_t s = blk_seq[gb];
	const uint64_t b = gb - blk_off[s];
	// halo blocks start no window
	if(b >= nblk_real[s]){ valid[gb] = 0; return; }
	const uint4 lo = planes[gb];
	const uint4 hi = planes[gb + 1];   // exists: every sequence has two halo blocks
	// per-position base multiplicity planes
	uint32_t nzl, d2l, d3l, d4l, cgl, nzh, d2h, d3h, d4h, cgh;
	{
		const uint32_t x = lo.x ^ lo.y, y = lo.x & lo.y, u = lo.z ^ lo.w, v = lo.z & lo.w;
		const uint32_t ones = x ^ u, c1 = x & u;
		const uint32_t twos = y ^ v ^ c1;
		const uint32_t fours = (y & v) | (c1 & (y ^ v));
		nzl = lo.x | lo.y | lo.z | lo.w;
		d2l = ~ones & twos & ~fours; d3l = ones & twos; d4l = fours;
		cgl = lo.y | lo.z;
	}
	{
		const uint32_t x = hi.x ^ hi.y, y = hi.x & hi.y, u = hi.z ^ hi.w, v = hi.z & hi.w;
		const uint32_t ones = x ^ u, c1 = x & u;
		const uint32_t twos = y ^ v ^ c1;
		const uint32_t fours = (y & v) | (c1 & (y ^ v));
		nzh = hi.x | hi.y | hi.z | hi.w;
		d2h = ~ones & twos & ~fours; d3h = ones & twos; d4h = fours;
		cgh = hi.y | hi.z;
	}
	uint32_t out = 0;
	for(uint32_t j = 0;j < 32;++j){
		if(funnel(nzl, nzh, j) != 0xFFFFFFFFu) continue;
		const uint32_t ngc = __popc(funnel(cgl, cgh, j));
		if(!((gc_ok >> ngc) & 1ull)) continue;
		const uint32_t n2 = __popc(funnel(d2l, d2h, j));
		const uint32_t n3 = __popc(funnel(d3l, d3h, j));
		const uint32_t n4 = __popc(funnel(d4l, d4h, j));
		// Word::degeneracy() > thr, exact integer form (pcr_host.hpp: degeneracy_exceeds)
		const uint32_t e = n2 + 2*n4;
		bool exceeds;
		if(e >= 33){ exceeds = true; }
		else{
			uint64_t p3 = 1;
			for(uint32_t k = 0;k < n3;++k) p3 *= 3;
			exceeds = p3 > ((uint64_t)max_degen >> e);
		}
		if(!exceeds) out |= (1u << j);
	}
	valid[gb] = out;
}

// ============================================================================== select_words
// Hits are appended to a fixed-capacity bucket per sequence (`cap` slots each), so the arg-max
// filter, the dedupe and the ordering by WordMatch::loc can be done per sequence by one workgroup
// (k_finalize) with no global sort.  counters[0]: overflow flag, counters[2]: largest bucket fill seen.
struct HitSink { uint32_t *best; Hit *hits; uint32_t *seq_count; uint32_t *counters; uint32_t cap; uint32_t ncand; uint32_t epoch; };
// counters[3] / touched[]: the sequences that received at least one hit, listed by k_touched after the scans
// (one wave-aggregated atomic per 64 sequences: appending from record_hit cost ~35 ns per touched sequence,
// all on one address -- more than the whole seed scan).
// best[] holds (pass epoch << 8) | count, so it never needs clearing: values of earlier passes compare lower.

__device__ __forceinline__ void record_hit_inline(const HitSink &k, uint32_t seq, uint32_t cand, uint64_t key, uint32_t cnt)
{
	const uint32_t tagged = (k.epoch << 8) | cnt;
	const uint32_t old = atomicMax(&k.best[(size_t)seq*k.ncand + cand], tagged);
	if(tagged >= old){
		const uint32_t slot = atomicAdd(&k.seq_count[seq], 1u);
		if(slot < k.cap){
			Hit h; h.key = key; h.cand = cand; h.cnt = cnt;
			k.hits[(size_t)seq*k.cap + slot] = h;
		}
		else{ atomicOr(&k.counters[0], 1u); atomicMax(&k.counters[2], slot + 1); }
	}
}

// (by value: a reference would make every kernel spill its HitSink to scratch at entry -- 64 B per lane of HBM writes)
__device__ __noinline__ void record_hit(const HitSink k, uint32_t seq, uint32_t cand, uint64_t key, uint32_t cnt)
{
	record_hit_inline(k, seq, cand, key, cnt);
}

__device__ __forceinline__ uint64_t make_key(uint32_t seq, int32_t loc, uint32_t strand /*1|2*/, uint32_t kind, uint32_t ord)
{
	return ((uint64_t)seq << KEY_SEQ_SHIFT) | ((uint64_t)(uint32_t)(loc + LOC_BIAS) << KEY_LOC_SHIFT) |
		((uint64_t)(strand - 1) << 7) | ((uint64_t)kind << 6) | ord;
}

__global__ void k_touched(const uint32_t *__restrict__ seq_count, uint32_t n, uint32_t *__restrict__ counters, uint32_t *__restrict__ touched)
{
	const uint32_t s = blockIdx.x*blockDim.x + threadIdx.x;
	const uint32_t fill = (s < n) ? seq_count[s] : 0u;
	const bool has = fill > 0;
	const uint64_t mask = __ballot(has);
	if(!mask) return;
	const uint32_t lane = threadIdx.x & 63u, leader = (uint32_t)__builtin_ctzll(mask);
	{   // counters[2]: the largest bucket fill of the pass (the host shrinks oversized buckets before the next pass)
		uint32_t mx = fill;
		for(int d = 32;d > 0;d >>= 1) mx = max(mx, (uint32_t)__shfl_xor((int)mx, d));
		if(lane == leader) atomicMax(&counters[2], mx);
	}
	uint32_t base = 0;
	if(lane == leader) base = atomicAdd(&counters[3], (uint32_t)__builtin_popcountll(mask));
	base = __shfl(base, leader);
	if(has) touched[base + (uint32_t)__builtin_popcountll(mask & ((1ull << lane) - 1ull))] = s;
}

// the same list from the DB's segment ends (a sequence with hits has at least one entry), for DBs whose per-sequence fills
// the fused tail has already zeroed
__global__ void k_touched_seg(const uint32_t *__restrict__ seg_hi, uint32_t n, uint32_t *__restrict__ counters, uint32_t *__restrict__ touched)
{
	const uint32_t s = blockIdx.x*blockDim.x + threadIdx.x;
	const bool has = s < n && seg_hi[s] != 0;
	const uint64_t mask = __ballot(has);
	if(!mask) return;
	const uint32_t lane = threadIdx.x & 63u, leader = (uint32_t)__builtin_ctzll(mask);
	uint32_t base = 0;
	if(lane == leader) base = atomicAdd(&counters[3], (uint32_t)__builtin_popcountll(mask));
	base = __shfl(base, leader);
	if(has) touched[base + (uint32_t)__builtin_popcountll(mask & ((1ull << lane) - 1ull))] = s;
}

// v1 match scan: one lane = one window start; the window's four 32-bit plane slices live in
// registers; candidates are wave-uniform (scalar loads), 4 and/or + popcount + compare each.
__global__ __launch_bounds__(SCAN_THREADS) void k_scan(
	const uint4 *__restrict__ planes, const uint32_t *__restrict__ valid,
	const uint64_t *__restrict__ blk_off, const uint64_t *__restrict__ len, const uint8_t *__restrict__ active,
	const uint32_t *__restrict__ tile_seq, const uint32_t *__restrict__ tile_pos0,
	const uint4 *__restrict__ cand_fwd, const uint4 *__restrict__ cand_rc, const uint32_t *__restrict__ cand_floor,
	uint32_t ncand, HitSink sink)
{
	const uint32_t tile = blockIdx.x;
	const uint32_t seq = tile_seq[tile];
	if(!active[seq]) return;
	const uint64_t L = len[seq];
	const uint64_t base = blk_off[seq];
	const uint32_t p0 = tile_pos0[tile];

	uint32_t wa[SCAN_NPOS], wc[SCAN_NPOS], wg[SCAN_NPOS], wt[SCAN_NPOS], ok[SCAN_NPOS];
#pragma unroll
	for(int i = 0;i < SCAN_NPOS;++i){
		const uint32_t p = p0 + threadIdx.x + SCAN_THREADS*i;
		wa[i] = wc[i] = wg[i] = wt[i] = 0; ok[i] = 0;
		if((uint64_t)p + 32 <= L){
			const uint32_t b = p >> 5, sh = p & 31;
			const uint4 lo = planes[base + b];
			const uint4 hi = planes[base + b + 1];
			wa[i] = funnel(lo.x, hi.x, sh); wc[i] = funnel(lo.y, hi.y, sh);
			wg[i] = funnel(lo.z, hi.z, sh); wt[i] = funnel(lo.w, hi.w, sh);
			ok[i] = (valid[base + b] >> sh) & 1u;
		}
	}

	for(uint32_t c = 0;c < ncand;++c){
		const uint4 mf = cand_fwd[c];
		const uint4 mr = cand_rc[c];
		const uint32_t fl = cand_floor[c];
#pragma unroll
		for(int i = 0;i < SCAN_NPOS;++i){
			const uint32_t cf = match_count(wa[i], wc[i], wg[i], wt[i], mf);
			const uint32_t cr = match_count(wa[i], wc[i], wg[i], wt[i], mr);
			if((cf >= fl || cr >= fl) && ok[i]){
				const int32_t p = (int32_t)(p0 + threadIdx.x + SCAN_THREADS*i);
				if(cf >= fl) record_hit(sink, seq, c, make_key(seq, p, 1, 0, 0), cf);       // sequence.cpp:184
				if(cr >= fl) record_hit(sink, seq, c, make_key(seq, p + 31, 2, 0, 0), cr);  // sequence.cpp:190
			}
		}
	}
}

// Irregular words: every lane keeps IRR_PER_LANE words in registers; the candidates are walked in the
// outer loop, so their planes and floors are wave-uniform (scalar loads, SGPR operands): 4 and/or +
// popcount + compare per (word, candidate).  grid.x = ceil(n_live / (IRR_THREADS*IRR_PER_LANE)).
constexpr int IRR_THREADS = 256, IRR_PER_LANE = 2;
struct IrrArgs { const IrrDev *irr; const uint32_t *perm; uint32_t n_live; uint32_t off_mask; /* slot offsets used by forward seeds */ };

// the work of irregular-scan workgroup `block` (IRR_THREADS lanes)
__device__ __forceinline__ void scan_irr_block(uint32_t block, const IrrDev *__restrict__ irr, const uint32_t *__restrict__ perm, uint32_t n_live,
	const uint8_t *__restrict__ active, const uint4 *__restrict__ cand_fwd, const uint32_t *__restrict__ cand_floor, uint32_t ncand,
	const HitSink &sink)
{
	uint32_t wa[IRR_PER_LANE], wc[IRR_PER_LANE], wg[IRR_PER_LANE], wt[IRR_PER_LANE];
	const uint32_t i0 = block*(IRR_THREADS*IRR_PER_LANE) + threadIdx.x;
#pragma unroll
	for(int k = 0;k < IRR_PER_LANE;++k){
		const uint32_t i = i0 + k*IRR_THREADS;
		wa[k] = wc[k] = wg[k] = wt[k] = 0;               // an empty word matches nothing (floors are >= 1 here, see below)
		if(i < n_live){                                  // the words whose size counter reaches min_oligo_length (sequence.cpp:157,239)
			const IrrDev e = irr[perm[i]];
			if(active[e.seq]){ wa[k] = e.w.a; wc[k] = e.w.c; wg[k] = e.w.g; wt[k] = e.w.t; }
		}
	}
#pragma unroll 8
	for(uint32_t c = 0;c < ncand;++c){
		const uint4 m = cand_fwd[c];
		const uint32_t fl = max(cand_floor[c], 1u);      // floor 0 ("everything matches") still needs one matching slot to exist as a word
		const bool zero_floor = cand_floor[c] == 0;
#pragma unroll
		for(int k = 0;k < IRR_PER_LANE;++k){
			const uint32_t cnt = match_count(wa[k], wc[k], wg[k], wt[k], m);
			if(cnt >= fl || (zero_floor && (wa[k] | wc[k] | wg[k] | wt[k]))){
				const IrrDev e = irr[perm[i0 + k*IRR_THREADS]];
				record_hit(sink, e.seq, c, make_key(e.seq, e.loc, e.meta & 0xFF, 1, (e.meta >> 16) & 0xFF), cnt);
			}
		}
	}
}

__global__ __launch_bounds__(IRR_THREADS) void k_scan_irr(const IrrDev *__restrict__ irr, const uint32_t *__restrict__ perm, uint32_t n_live,
	const uint8_t *__restrict__ active, const uint4 *__restrict__ cand_fwd, const uint32_t *__restrict__ cand_floor, uint32_t ncand,
	HitSink sink)
{
	scan_irr_block(blockIdx.x, irr, perm, n_live, active, cand_fwd, cand_floor, ncand, sink);
}

// LDS hand-off between lanes of ONE wave: order the wave's own LDS traffic, no workgroup barrier
__device__ __forceinline__ void wave_sync() { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier(); }

#include "pcr_scan_bitsliced.inc"
#include "pcr_scan_seed.inc"
#include "pcr_scan_seed2.inc"
#include "pcr_scan_seed3.inc"

// One workgroup per sequence: keep the hits that attain the final per-(sequence,candidate) maximum
// (select_words.cpp:100-117), sort them by (loc, strand, kind, ord) (bitonic, LDS), drop duplicates
// (the union over candidates, select_words.cpp:126-128) and materialise the DB entries of the
// sequence into its slot range [seq*cap, seq*cap + n).  seg_hi[seq] = seq*cap + n.
constexpr int FIN_WAVES = 8;          // one wave per sequence, 8 sequences per workgroup (1 when the buckets outgrow 1024 hits: LDS)
constexpr uint32_t MAX_BUCKET_CAP = 8192;   // 8192 keys x 8 B = the 64 KB of LDS one wave may sort in


// (seq_base: blk_off of the key's sequence, which callers that work on one sequence have loaded long before)
__device__ __forceinline__ void materialise_entry_at(uint64_t k, const uint4 *__restrict__ planes, uint64_t seq_base,
	const IrrDev *__restrict__ irr, const uint32_t *__restrict__ irr_off, DevEntry &e)
{
	const uint32_t seq = (uint32_t)(k >> KEY_SEQ_SHIFT);
	const int32_t loc = (int32_t)(uint32_t)((k >> KEY_LOC_SHIFT) & 0xFFFFFFFFull) - LOC_BIAS;
	const uint32_t strand = (uint32_t)((k >> 7) & 1) + 1;
	const uint32_t kind = (uint32_t)((k >> 6) & 1), ord = (uint32_t)(k & 63);
	e.loc = loc; e.seq = seq; e.strand = strand; e.pad = 0;
	if(kind == 0){
		const uint32_t p = (strand == 1) ? (uint32_t)loc : (uint32_t)(loc - 31);
		const uint32_t b = p >> 5, sh = p & 31;
		const uint4 lo = planes[seq_base + b];
		const uint4 hi = planes[seq_base + b + 1];
		const uint32_t a = funnel(lo.x, hi.x, sh), c = funnel(lo.y, hi.y, sh);
		const uint32_t g = funnel(lo.z, hi.z, sh), t = funnel(lo.w, hi.w, sh);
		if(strand == 1){ e.w.a = a; e.w.c = c; e.w.g = g; e.w.t = t; }
		else{ e.w.a = __brev(t); e.w.t = __brev(a); e.w.c = __brev(g); e.w.g = __brev(c); }   // Word::complement, word.h:140
	}
	else{
		e.w.a = e.w.c = e.w.g = e.w.t = 0;
		for(uint32_t j = irr_off[seq];j < irr_off[seq + 1];++j){
			const IrrDev r = irr[j];
			if(r.loc == loc && (r.meta & 0xFF) == strand && ((r.meta >> 16) & 0xFF) == ord){ e.w = r.w; break; }
		}
	}
}

__device__ void materialise_entry(uint64_t k, const uint4 *__restrict__ planes, const uint64_t *__restrict__ blk_off,
	const IrrDev *__restrict__ irr, const uint32_t *__restrict__ irr_off, DevEntry &e)
{
	const uint32_t seq = (uint32_t)(k >> KEY_SEQ_SHIFT);
	const int32_t loc = (int32_t)(uint32_t)((k >> KEY_LOC_SHIFT) & 0xFFFFFFFFull) - LOC_BIAS;
	const uint32_t strand = (uint32_t)((k >> 7) & 1) + 1;
	const uint32_t kind = (uint32_t)((k >> 6) & 1), ord = (uint32_t)(k & 63);
	e.loc = loc; e.seq = seq; e.strand = strand; e.pad = 0;
	if(kind == 0){
		const uint32_t p = (strand == 1) ? (uint32_t)loc : (uint32_t)(loc - 31);
		const uint32_t b = p >> 5, sh = p & 31;
		const uint4 lo = planes[blk_off[seq] + b];
		const uint4 hi = planes[blk_off[seq] + b + 1];
		const uint32_t a = funnel(lo.x, hi.x, sh), c = funnel(lo.y, hi.y, sh);
		const uint32_t g = funnel(lo.z, hi.z, sh), t = funnel(lo.w, hi.w, sh);
		if(strand == 1){ e.w.a = a; e.w.c = c; e.w.g = g; e.w.t = t; }
		else{ e.w.a = __brev(t); e.w.t = __brev(a); e.w.c = __brev(g); e.w.g = __brev(c); }   // Word::complement, word.h:140
	}
	else{
		// the irregular word with this (loc, strand, ord) in the sequence's list
		e.w.a = e.w.c = e.w.g = e.w.t = 0;
		for(uint32_t j = irr_off[seq];j < irr_off[seq + 1];++j){
			const IrrDev r = irr[j];
			if(r.loc == loc && (r.meta & 0xFF) == strand && ((r.meta >> 16) & 0xFF) == ord){ e.w = r.w; break; }
		}
	}
}

// ALL (pcr_select_sites): every hit is kept -- no arg-max filter, best[] is not read (it may be NULL).
template<int WAVES, bool ALL = false>
__global__ __launch_bounds__(64*WAVES) void k_finalize(const Hit *__restrict__ hits, const uint32_t *__restrict__ seq_count,
	uint32_t cap, const uint32_t *__restrict__ best, uint32_t ncand, const uint4 *__restrict__ planes,
	const uint64_t *__restrict__ blk_off, const IrrDev *__restrict__ irr, const uint32_t *__restrict__ irr_off,
	DevEntry *__restrict__ db, uint32_t *__restrict__ seg_hi, uint32_t *__restrict__ counters, uint32_t epoch,
	const uint32_t *__restrict__ touched)
{
	extern __shared__ __attribute__((aligned(16))) uint64_t fin_lds[];   // WAVES x np2cap keys
	__shared__ uint32_t part_all[64*WAVES];
	const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
	uint32_t np2cap = 1; while(np2cap < cap) np2cap <<= 1;
	// only sequences that received hits (seg_hi of the others stays 0 = empty).  One workgroup per 8 sequences of
	// the whole set; 256 fat workgroups walking the list were slower (10.7 vs 7.4 us at C2: latency-, not dispatch-bound)
	for(uint32_t t_idx = blockIdx.x*WAVES + wave;t_idx < counters[3];t_idx += gridDim.x*WAVES){
	const uint32_t seq = touched[t_idx];
	uint64_t *fin_keys = fin_lds + (size_t)wave*np2cap;
	uint32_t *part = part_all + wave*64;
	const uint32_t n = min(seq_count[seq], cap);
	uint32_t np2 = 1; while(np2 < n) np2 <<= 1;
	for(uint32_t i = lane;i < np2;i += 64){
		uint64_t k = ~0ull;
		if(i < n){
			const Hit h = hits[(size_t)seq*cap + i];
			if constexpr (ALL) k = h.key;
			else if(((epoch << 8) | h.cnt) == best[(size_t)seq*ncand + h.cand]) k = h.key;
		}
		fin_keys[i] = k;
	}
	wave_sync();
	for(uint32_t k = 2;k <= np2;k <<= 1){
		for(uint32_t j = k >> 1;j > 0;j >>= 1){
			for(uint32_t i = lane;i < np2;i += 64){
				const uint32_t l = i ^ j;
				if(l > i){
					const uint64_t a = fin_keys[i], b = fin_keys[l];
					const bool up = ((i & k) == 0);
					if((a > b) == up){ fin_keys[i] = b; fin_keys[l] = a; }
				}
			}
			wave_sync();
		}
	}
	// distinct, non-sentinel keys -> ranks (each lane owns a contiguous chunk)
	const uint32_t chunk = (np2 + 63)/64;
	const uint32_t lo = lane*chunk, hi = min(np2, lo + chunk);
	uint32_t cnt = 0;
	for(uint32_t i = lo;i < hi;++i){
		const uint64_t k = fin_keys[i];
		if(k != ~0ull && (i == 0 || fin_keys[i - 1] != k)) ++cnt;
	}
	part[lane] = cnt;
	wave_sync();
	if(lane == 0){
		uint32_t run = 0;
		for(int t = 0;t < 64;++t){ const uint32_t c = part[t]; part[t] = run; run += c; }
		seg_hi[seq] = seq*cap + run;
	}
	wave_sync();
	uint32_t rank = part[lane];
	for(uint32_t i = lo;i < hi;++i){
		const uint64_t k = fin_keys[i];
		if(k != ~0ull && (i == 0 || fin_keys[i - 1] != k)){
			DevEntry e;
			materialise_entry(k, planes, blk_off, irr, irr_off, e);
			db[(size_t)seq*cap + rank] = e;
			++rank;
		}
	}
	wave_sync();                                 // the wave's LDS keys are reused by its next sequence
	}
}

// Buckets beyond MAX_BUCKET_CAP (low-complexity sequence against low-complexity oligos: thousands of tied
// windows): the same filter / sort / dedupe / materialise with the keys in global scratch and one
// 256-thread workgroup per touched sequence.  Slow path; exists so that such inputs are not refused.
constexpr int FINBIG_THREADS = 256;
constexpr uint32_t MAX_BUCKET_CAP_GLOBAL = 65536;
template<bool ALL = false>
__global__ __launch_bounds__(FINBIG_THREADS) void k_finalize_big(const Hit *__restrict__ hits, const uint32_t *__restrict__ seq_count,
	uint32_t cap, const uint32_t *__restrict__ best, uint32_t ncand, const uint4 *__restrict__ planes,
	const uint64_t *__restrict__ blk_off, const IrrDev *__restrict__ irr, const uint32_t *__restrict__ irr_off,
	DevEntry *__restrict__ db, uint32_t *__restrict__ seg_hi, uint32_t *__restrict__ counters, uint32_t epoch,
	const uint32_t *__restrict__ touched, uint64_t *__restrict__ scratch)
{
	__shared__ uint32_t part[FINBIG_THREADS];
	if(blockIdx.x >= counters[3]) return;
	const uint32_t seq = touched[blockIdx.x], tid = threadIdx.x;
	uint32_t np2cap = 1; while(np2cap < cap) np2cap <<= 1;
	uint64_t *fin_keys = scratch + (size_t)blockIdx.x*np2cap;
	const uint32_t n = min(seq_count[seq], cap);
	uint32_t np2 = 1; while(np2 < n) np2 <<= 1;
	for(uint32_t i = tid;i < np2;i += FINBIG_THREADS){
		uint64_t k = ~0ull;
		if(i < n){
			const Hit h = hits[(size_t)seq*cap + i];
			if constexpr (ALL) k = h.key;
			else if(((epoch << 8) | h.cnt) == best[(size_t)seq*ncand + h.cand]) k = h.key;
		}
		fin_keys[i] = k;
	}
	__syncthreads();
	for(uint32_t k = 2;k <= np2;k <<= 1){
		for(uint32_t j = k >> 1;j > 0;j >>= 1){
			for(uint32_t i = tid;i < np2;i += FINBIG_THREADS){
				const uint32_t l = i ^ j;
				if(l > i){
					const uint64_t a = fin_keys[i], b = fin_keys[l];
					const bool up = ((i & k) == 0);
					if((a > b) == up){ fin_keys[i] = b; fin_keys[l] = a; }
				}
			}
			__syncthreads();
		}
	}
	const uint32_t chunk = (np2 + FINBIG_THREADS - 1)/FINBIG_THREADS;
	const uint32_t lo = min(np2, tid*chunk), hi = min(np2, lo + chunk);
	uint32_t cnt = 0;
	for(uint32_t i = lo;i < hi;++i){
		const uint64_t k = fin_keys[i];
		if(k != ~0ull && (i == 0 || fin_keys[i - 1] != k)) ++cnt;
	}
	part[tid] = cnt;
	__syncthreads();
	if(tid == 0){
		uint32_t run = 0;
		for(int t = 0;t < FINBIG_THREADS;++t){ const uint32_t c = part[t]; part[t] = run; run += c; }
		seg_hi[seq] = seq*cap + run;
	}
	__syncthreads();
	uint32_t rank = part[tid];
	for(uint32_t i = lo;i < hi;++i){
		const uint64_t k = fin_keys[i];
		if(k != ~0ull && (i == 0 || fin_keys[i - 1] != k)){
			DevEntry e;
			materialise_entry(k, planes, blk_off, irr, irr_off, e);
			db[(size_t)seq*cap + rank] = e;
			++rank;
		}
	}
}

#include "pcr_screen.inc"

#include "pcr_sw.inc"
#include "pcr_thermo.inc"

// ============================================================================== host state
constexpr uint32_t N_TOUCHED_UNKNOWN = 0xFFFFFFFFu;
constexpr uint32_t EPOCH_LIMIT = (1u << 24) - 1;    // largest pass epoch that fits the 24-bit tag of best[]

struct SeqSet {
	uint32_t n = 0;
	std::vector<std::vector<uint8_t> > packed;   // host copy (split_sequence, irregular re-derivation)
	std::vector<uint64_t> len, blk_off, nblk_real;
	std::vector<float> weight; DevBuf<float> d_weight; bool weight_dirty = true;   // device copy on demand (pcr_optimize_batch)
	std::vector<uint8_t> active;
	std::vector<std::vector<pcrhost::IrrEntry> > irr_host;
	uint64_t total_blocks = 0;
	uint32_t n_tiles = 0, n_irr = 0;
	bool ctrl_clean = false;     // counters[0], counters[2], the per-sequence fills and the segment ends of sequences without hits are zero (the fused tail k_post leaves them so; counters[1] and [3] may be set by k_post / k_touched*: the lean k_seed2 zeroes those two itself): the next fused pass need not clear the block
	bool touched_from_seg = false;   // the per-sequence fills were zeroed by k_post: the touched list comes from the segment ends
	uint32_t bucket_cap = 64;   // hit slots per sequence of this set's word DB (grows on overflow; per set: the target DB at 0.9 needs 64, a background DB selected at 0.72 thousands)
	DevBuf<uint32_t> irr_perm; uint32_t irr_size_count[256];   // irregular words by size counter, largest first
	DevBuf<uint4> planes;
	DevBuf<uint32_t> valid, nib, tb, blk_seq, tile_seq, tile_pos0, irr_off, degen_tiles;
	// valid[] and tb[] carry zero padding in front and behind (k_seed2's tile fetch has no bounds checks, pcr_scan_seed2.inc): the DATA start here
	uint32_t *valid_d() const { return valid.p + S2_VALID_FRONT; }
	uint32_t *tb_d() const { return tb.p + S2_TB_FRONT; }
	DevBuf<uint8_t> tile_degen; uint32_t n_degen_tiles = 0;
	DevBuf<TileDesc> tile_desc;   // one per tile, with the sequence's active flag folded in (k_tile_desc; refreshed by pcr_set_active)
	DevBuf<uint64_t> d_len, d_blk_off, d_nblk_real;
	DevBuf<uint8_t> d_active;
	std::vector<uint8_t> has_eos; DevBuf<uint8_t> d_has_eos;   // sequence holds an EOS nibble (record padding, splits): only then has_split has to look
	DevBuf<IrrDev> irr;
	DevBuf<IrrScan> irr_scan;     // the irregular words in scan order with their 2-bit codes (k_seed2)
	DevBuf<uint32_t> irx_first, irx_last, irx_words, irx_sums; bool irx_valid = false, irx_usable = false;   // their inverse index (pcr_scan_seed2.inc), built on demand; usable: no key's run is longer than IRX_MAX_RUN
	uint32_t irr_n_multi = 0;     // irregular words holding an IUPAC slot (they meet every candidate: no index for them)
	// the positions of the set by the 9-gram that starts there (pcr_scan_seed3.inc), built on demand after a load
	DevBuf<uint32_t> pix_first, pix_last, pix_sums, blk_info, blk_local, blk_tile0; DevBuf<uint4> pix_ent; std::vector<uint32_t> pix_start_h; uint64_t pix_generation = 0; bool pix_valid = false, pix_usable = false;
	DevBuf<uint8_t> codes; DevBuf<uint64_t> d_code_off; bool have_codes = false;
	// word DB of the last select
	bool have_db = false;
	uint32_t n_entries = 0;     // DB entries over all sequences
	uint32_t db_cap = 0;        // slots per sequence in `db`; the entries of sequence s are db[s*db_cap .. seg_hi[s])
	uint64_t n_slots = 0;       // n * db_cap
	DevBuf<DevEntry> db;
	DevBuf<uint32_t> touched;     // sequences holding DB entries (k_touched)
	DevBuf<uint32_t> ctrl;        // [0..7] counters | [8, 8+n) per-sequence hit counts | [8+n, 8+2n) seg_hi : one memset per pass
	uint32_t n_touched = 0;
	bool touched_built = false;   // touched[] / counters[3] hold the list of the last pass (the fused tail does not build it)
	uint32_t *d_seg_hi = nullptr;
};

} // namespace

// A few host threads that live as long as the handle (pcr_optimize.inc's loops over the assays of a batch).  run(): part indices
// 0 .. n_parts-1 are claimed one by one by the workers and by the calling thread, which returns when all are done.
struct HostPool {
	std::vector<std::thread> th;
	std::mutex m; std::condition_variable cv_go, cv_done;
	std::function<void(unsigned)> fn; unsigned n_parts = 0, next = 0, pending = 0; uint64_t gen = 0; bool stop = false;
	explicit HostPool(unsigned n_workers){ for(unsigned i = 0;i < n_workers;++i) th.emplace_back([this]{ work(); }); }
	~HostPool(){ { std::lock_guard<std::mutex> lk(m); stop = true; } cv_go.notify_all(); for(std::thread &t : th) t.join(); }
	unsigned size() const { return (unsigned)th.size(); }
	void work()
	{
		uint64_t seen = 0;
		std::unique_lock<std::mutex> lk(m);
		while(true){
			cv_go.wait(lk, [&]{ return stop || gen != seen; });
			if(stop) return;
			seen = gen;
			while(next < n_parts){ const unsigned p = next++; lk.unlock(); fn(p); lk.lock(); }
			if(--pending == 0) cv_done.notify_one();
		}
	}
	void run(unsigned parts, std::function<void(unsigned)> f)
	{
		std::unique_lock<std::mutex> lk(m);
		fn = std::move(f); n_parts = parts; next = 0; pending = (unsigned)th.size(); ++gen;
		cv_go.notify_all();
		while(next < n_parts){ const unsigned p = next++; lk.unlock(); fn(p); lk.lock(); }
		cv_done.wait(lk, [&]{ return pending == 0; });
	}
};

namespace { struct PassJob; struct Launcher; }   // pcr_select.inc

// Which of a handle's buffers a call's item stage (pcr_pool.inc) and melt stage (pcr_site_tm.inc) work in: the stages know no
// member names.  joff and res are the melt stage's; item_tm and flag go with its k_item_tm (NULL: the caller reduces the jobs itself).
struct ItemBufs {
	DevBuf<uint8_t> *tmp; DevBuf<uint32_t> *cnt; DevBuf<uint64_t> *eoff; DevBuf<uint2> *items;
	DevBuf<uint64_t> *joff; DevBuf<float4> *res; DevBuf<uint2> *item_tm; DevBuf<uint32_t> *flag;
};
// The scratch that the entry points which melt a pool's items and join them have in common: the uploaded tables, scan / sort
// scratch, per-entry / per-item counts, error flags, entry and job offsets, items, per-job results, per-item Tm, and the offsets of
// the items' products where the join counts products (ioff).  Nothing in it outlives the call that wrote it.
struct ItemScratch {
	DevBuf<uint8_t> in, tmp; DevBuf<uint32_t> cnt, flag; DevBuf<uint64_t> eoff, joff, ioff; DevBuf<uint2> items, item_tm; DevBuf<float4> res;
	ItemBufs bufs() { return ItemBufs{&tmp, &cnt, &eoff, &items, &joff, &res, &item_tm, &flag}; }
};

struct pcr_ctx {
	int device = 0;
	std::unique_ptr<HostPool> pool_;
	HostPool &host_pool()
	{
		if(!pool_){ const unsigned hw = std::max(1u, std::thread::hardware_concurrency()); pool_.reset(new HostPool(std::min(hw, 16u) - 1u)); }   // (a GPU box gives its process 16 cores)
		return *pool_;
	}
	// Every device resource below frees itself (pcr_owned.hpp).  The streams come first so that they are destroyed last, after
	// every buffer and event; pcr_destroy synchronises both before it deletes the handle.
	Stream stream;                      // created by pcr_create, or the caller's (borrowed: never destroyed here)
	Stream aux_stream;                  // the optimiser's thermodynamics run here, beside the coverage passes on `stream` (pcr_optimize.inc); created on first use
	std::string design_text;            // the output file of the last pcr_design call
	DevBuf<uint64_t> split_where;       // pcr_split_many's (block, bit) list
	pcr_params params;
	pcrhost::PackFilter filt;
	SeqSet sets[PCR_N_SETS];   // target, background, multiplex (accepted amplicons), scratch (pcr_multiplex_screen's trial amplicons)
	// scratch
	DevBuf<uint32_t> best, counters, mask, status;
	int scan_version = 3;
	bool force_seed1 = false;   // PCRAMP_SEED=1: the first form of the seed scan (A/B)
	// second and third forms of the seed scan: the per-oligo seed caches, their positional memos and the listing's scratch
	// (pcr_seed_lists.hpp; the pass's lists live in its PassJob: PlanLists, pcr_select.inc).  Caller-thread state: stage A alone
	// reads and writes it.  The third form has a cache of its own (the oligo's FOLDED seeds, pcrhost::orientation_fold_seeds, are other
	// lists under the same key), with a span byte per seed and the running 64-entry chunks of the seeds' spans in the sets whose
	// position index has one of the last S3_CHUNK_SETS generations.
	pcrseed::Lister seed_lists;                   // PCRAMP_SEED_MEMO=0: every orientation through the hash (A/B)
	static constexpr int S3_CHUNK_SETS = pcrseed::CHUNK_SETS;
	struct S2Key { uint32_t a, c, g, t, floor_; bool operator==(const S2Key &o) const { return a == o.a && c == o.c && g == o.g && t == o.t && floor_ == o.floor_; } };
	struct S2KeyHash { size_t operator()(const S2Key &k) const { uint64_t h = 0x9E3779B97F4A7C15ull; for(uint32_t v : {k.a, k.c, k.g, k.t, k.floor_}){ h ^= v; h *= 0x100000001B3ull; h ^= h >> 29; } return (size_t)h; } };
	struct S2Entry { std::vector<uint32_t> seeds; /* code | off << 16 */ uint32_t off_mask; bool seedable; };   // (first form: s1_cache)
	std::vector<pcrhost::Seed> s2_tmp;
	struct S3Launch { Seed3Slices W; uint32_t n_chunks, per_wg, slice_cap, n_irr_wg; };
	int pair_mode = 1; bool s3_pair_attr_set = false;   // PCRAMP_PAIR: 0 never pair two handles' passes into one launch (A/B), 1 by the backlog rule, 2 "force" (tests: hold until a partner, a flush or the time cap)
	bool no_seed3 = false, s3_attr_set = false;   // PCRAMP_SEED3=0: second form (A/B)
	bool s3_next = true;                          // PCRAMP_S3_NEXT=0: the third form with the plain 9-gram lists, span A..T: what it read before the index was sorted by the next base (A/B)
	bool s2_attr_set = false; uint32_t s2_dbg = 0; bool no_irr_index = false;   // PCRAMP_IRR_INDEX=0: the irregular words scanned in chunks by every wave (A/B)
	// first form, tables built on the device (k_seed_tables): the pass's seed list, its own per-oligo cache (8-gram seeds), the tables
	std::unordered_map<S2Key, S2Entry, S2KeyHash> s1_cache;
	DevBuf<uint32_t> s1_image, s1_heads, s1_multi, s1_part;
	bool host_seed_tables = false;   // PCRAMP_SEED_TABLES=host: build them on the host as for passes with shift candidates (A/B)
	DevBuf<Hit> hits;
	DevBuf<uint64_t> bits_fr, bits_rf;
	DevBuf<OligoDev> oligos;
	DevBuf<SwJob> sw_jobs; DevBuf<SwOut> sw_out; DevBuf<uint8_t> sw_q, sw_qlen, sw_t, entry_codes, entry_lens;
	DevBuf<AmpRec> amp_recs, amp_recs2; DevBuf<BgPairDev> bg_pairs;
	DevBuf<uint64_t> amp_keys; DevBuf<uint32_t> amp_pkeys, amp_pair_start; DevBuf<uint8_t> sort_tmp;   // reference-order sort of the candidate amplicons (order_amplicons)
	DevBuf<thermo::Job> th_jobs; DevBuf<thermo::JobOut> th_out; DevBuf<int> th_dg; DevBuf<uint2> th_map; DevBuf<uint32_t> th_bad;
	float th_dg_salt = -1.0f;   // salt the table in th_dg was built for
	DevBuf<unsigned long long> th_dbg; bool th_attr_set = false;
	std::vector<thermo::Job> th_host_jobs; std::vector<thermo::JobOut> th_host_res;   // pcr_thermo's job records and results, kept between calls
	MappedBuf<uint8_t> sw_pin; Event sw_done[2];   // pcr_sw_align_words: two pinned chunk buffers (words in, results out)
	DevBuf<pcr_amplicon> mx_amp;   // pcr_collect_amplicons records
	DevBuf<OligoDev> opt_oligos; DevBuf<uint2> opt_jobs; DevBuf<float> opt_cov; DevBuf<uint32_t> opt_loc, opt_tasks;   // pcr_optimize_batch: base oligos + trial words, per-oligo variant ranges, coverages
	DevBuf<Planes> mx_keys; uint32_t mx_n_keys = 0; DevBuf<uint32_t> mx_count;   // multiplex background: unique words of the accepted amplicons (pcr_multiplex.inc)
	// pcr_pool_products (pcr_pool.inc): oligo table + intended bitmap, per-entry / per-item counts and offsets, items, records, sort keys
	DevBuf<uint8_t> pool_in, pool_tmp; DevBuf<uint32_t> pool_cnt, pool_ord; DevBuf<uint64_t> pool_eoff, pool_ioff, pool_keys; DevBuf<uint2> pool_items; DevBuf<pcr_product> pool_rec;
	// pcr_site_tm (pcr_site_tm.inc): oligo tables, per-entry counts and offsets, items, per-item job offsets, per-job results, sort keys and order, records
	DevBuf<uint8_t> site_in, site_tmp; DevBuf<uint32_t> site_cnt, site_ord, site_flag; DevBuf<uint64_t> site_eoff, site_joff, site_keys; DevBuf<uint2> site_items; DevBuf<float4> site_res; DevBuf<pcr_site> site_rec;
	bool site_attr_set = false;
	// pcr_site_variants (pcr_site_variants.inc; it also uses site_*): what each item spells, the key order, each item's variant, variant starts,
	// records (key order | record order), the variants' sort keys and orders (+ their rank), the site map
	DevBuf<uint8_t> sv_item; DevBuf<uint32_t> sv_ord, sv_var, sv_start, sv_vord, sv_map; DevBuf<pcr_site_variant> sv_rec; DevBuf<uint64_t> sv_vkeys;
	bool sv_attr_set = false;
	// pcr_site_repair (pcr_site_repair.inc; on top of the variant pipeline's site_* and sv_*): footprints, (oligo, sequence) pair keys + the
	// held bitset, the uint32 tables (sites, ranges, pairs, runs, candidates), per-oligo state + candidate scores, the step records
	DevBuf<uint4> rp_foot; DevBuf<uint64_t> rp_keys; DevBuf<uint32_t> rp_u32; DevBuf<uint8_t> rp_state; DevBuf<pcr_repair_step> rp_rec;
	// an attached target shard (pcr_shard_targets, pcr_shard.inc): PCR_SET_TARGET holds rows [shard_first, shard_first + n) of
	// shard_n_total, and the local search combines target coverage over shard_comm; NULL = not sharded
	pcr_comm *shard_comm = nullptr; uint64_t shard_first = 0, shard_n_total = 0; int shard_mode = 0;
	DevBuf<uint64_t> sh_rec, sh_full; DevBuf<uint8_t> sh_stage;   // the combine's record, the gathered records, staging of host collectives on RCCL
	std::vector<uint64_t> shard_bounds; DevBuf<uint64_t> d_shard_bounds;   // every rank's first row, rank order, and n_total last (world + 1)
	// the design loop over a shard (pcr_shard_sampler_targets): rank 0's host-only copy of the whole target set for the sampler
	// (packed 4 bits per base as loaded, EOS splits applied as the loop makes them; empty on the other ranks)
	bool design_ready = false; DevBuf<uint64_t> sh_bits;   // (and the best assay's local + global bits)
	std::vector<std::vector<uint8_t> > samp_packed; std::vector<uint64_t> samp_len;
	void drop_shard(){ shard_comm = nullptr; shard_mode = 0; shard_bounds.clear(); design_ready = false; samp_packed.clear(); samp_len.clear(); }
	// the reference's MPI mode (pcr_design_trial_ranks, pcr_trial_ranks.inc): every rank holds the whole sets, pcr_design samples
	// this rank's trials and reduces the ranks' best assays over trial_comm; NULL = not attached
	pcr_comm *trial_comm = nullptr;
	size_t amp_cap = size_t(1) << 20;
	uint32_t n_cu = 256;        // compute units of the device (hipDeviceProp)
	DevBuf<uint64_t> fin_scratch;   // k_finalize_big's keys
	std::vector<uint16_t> seed_count; std::vector<uint8_t> seed_fill, seed_own;   // host scratch of the seed-table builder
	uint32_t epoch = 0;         // pass counter tagging best[] (see HitSink)
	uint32_t debug_epoch = 0;   // PCRAMP_DEBUG_EPOCH: value the counter takes when best[] is first cleared
	bool opt_pm_global = false;   // PCRAMP_OPT_PM=global: k_pair_moves_batch (partner walk through global memory) instead of k_pair_moves_lds (A/B)
	uint32_t opt_dbg_wg_tasks = 0, opt_dbg_task_cap = 0;   // PCRAMP_DEBUG_OPT_TASKS=<per workgroup>,<global>: shrink k_pair_moves_batch's task lists so that their overflow branches run (tests)
	uint64_t best_seen = 0;      // generation of best[] that has been cleared (the allocator may hand the same address back: never compare pointers)
	// pinned staging for the small per-call host->device payload (candidates, tables, oligos): one async copy
	// ring of host-mapped staging buffers: a slot is rewritten only after the k_stage that read it has run,
	// so the host can prepare the next pass while the previous one is still on the GPU
	static constexpr int STAGE_RING = 4;
	struct StageSlot { MappedBuf<uint8_t> buf; Event done; bool busy = false;
	                   uint32_t guard_seq = 0; /* != 0: free once the pass with this mailbox sequence number has published */ };
	StageSlot stage[STAGE_RING]; int stage_next = 0;
	// The lean form of the fused pass needs no staging launch at all: its tables are written by the CPU straight into
	// fine-grained DEVICE memory (large BAR: posted writes, ordered before the doorbell of the launch that follows; measured
	// 0.6 us for 32 KB, profiles/microbench/bar_write.hip), a ring of its own because the kernels read the slot itself.
	struct DirectSlot { DevBuf<uint8_t> buf{true}; uint32_t guard_seq = 0; };
	DirectSlot dstage[STAGE_RING]; int dstage_next = 0;
	bool direct_ok = false;       // fine-grained device memory can be had and written (probed in pcr_create; PCRAMP_STAGE=kernel turns it off)
	typedef PassMail Mail;
	static constexpr uint32_t MAIL_RING = 8;
	MappedBuf<Mail> mail;   // host-mapped ring (slot = seq % MAIL_RING): k_publish writes it, the host spins on seq
	uint32_t mail_seq = 0;
	// results of the small synchronous calls (move coverage, thermodynamics) come back the same way: a kernel
	// copies them into a host-mapped buffer and raises a flag the host spins on (no copy-engine packets, no
	// interrupt wake-up; three pageable hipMemcpyAsync + a stream sync cost ~1.8 ms per call instead)
	MappedBuf<uint8_t> ret;
	MappedBuf<uint8_t> in;   // the way in for small synchronous calls: a mapped buffer the kernel reads directly (the call waits for its results, so one buffer is enough)
	MappedBuf<uint32_t> ret_flag; uint32_t ret_seq = 0;
	// passes enqueued by pcr_screen_device whose counters have not been looked at yet (pcr_synchronize / any
	// other entry point drains them; a bucket overflow found then replays the passes synchronously)
	struct Pending {
		uint32_t seq; int which; std::vector<pcr_pair> pairs; int opt5, opt3; float thr; uint32_t min_len;
		pcr_amplify_args args; uint64_t *d_fr, *d_rf;
	};
	std::vector<Pending> pending;
	std::vector<std::vector<pcr_pair> > pair_pool;   // pair lists of drained passes, recycled by the next ones (caller thread)
	// The default pcr_screen_device pass is planned on the caller's thread and staged and launched by the stream's launcher thread
	// (pcr_select.inc: PassJob lists who owns what meanwhile).  launcher: attached by the first pipelined pass, shared by the handles
	// of the stream; lq_client: this handle's jobs in its queue and the error of one that failed.
	bool launch_thread = true;                    // PCRAMP_LAUNCH_THREAD=0: every pass runs inline on the caller's thread
	Launcher *launcher = nullptr; pcrq::Client lq_client; uint64_t n_pipelined = 0;
	std::mutex job_m; std::vector<PassJob *> job_free, job_all;   // recycled pass jobs (job_free under job_m: the launcher thread hands them back)
	DevBuf<uint8_t> arena;
	const uint4 *d_cand_fwd = nullptr, *d_cand_rc = nullptr; const uint32_t *d_cand_floor = nullptr;
	const OligoDev *d_oligos = nullptr;
	// host-side phase timers (PCRAMP_TIMING=1: printed by pcr_destroy)
	bool debug_log = false;                       // PCRAMP_DEBUG: plan / launch lines on stderr (read once: getenv walks the environment)
	bool timing = false; double t_host[8] = {0, 0, 0, 0, 0, 0, 0, 0}; uint64_t n_timed = 0;
	// profiling
	bool prof = false; uint32_t prof_stride = 1, prof_pass = 0;   // events bracket the scan of every prof_stride-th pass
	std::vector<std::pair<Event, Event> > prof_events;
	double prof_ms = 0.0; uint64_t prof_launches = 0;
	// the same for the other kernels bench.py prices (PCR_PROF_SW, PCR_PROF_THERMO): every launch while profiling is on
	std::vector<std::pair<Event, Event> > prof_events_k[PCR_PROF_KERNELS];
	double prof_ms_k[PCR_PROF_KERNELS] = {0.0, 0.0, 0.0}; uint64_t prof_launches_k[PCR_PROF_KERNELS] = {0, 0, 0};
	// pcr_pool_dimers (pcr_pool_dimers.inc): oligo table + prefixes + log strands, scan scratch, per-duplex results, per-cell records and the kept ones, keep flags and their scan, error flag.
	// (Last, so that every member above keeps its place: the screen pass is host-bound and two threads share this struct.)
	DevBuf<uint8_t> pdim_in, pdim_tmp; DevBuf<float4> pdim_res; DevBuf<pcr_pool_dimer> pdim_rec, pdim_out; DevBuf<uint32_t> pdim_keep, pdim_off, pdim_flag;
	bool pdim_attr_set = false;
	// pcr_pool_products_tm (pcr_products_tm.inc), beside the shared set at the end (`shared`): the pool's bit rows, records, sort keys and order.
	// (After pdim_*, for the same reason; so is everything below.)
	DevBuf<uint32_t> ptm_ord; DevBuf<uint64_t> ptm_keys, ptm_bits; DevBuf<pcr_product_tm> ptm_rec;
	// pcr_pool_probe_hits (pcr_probe_hits.inc), beside `shared`: the kept products (two item indices and two DB slots each), the hit
	// counts and offsets per product, the detected rows, hit records, sort keys and order.
	DevBuf<uint32_t> pph_hcnt, pph_ord; DevBuf<uint64_t> pph_hoff, pph_keys, pph_bits; DevBuf<uint4> pph_prod; DevBuf<pcr_probe_hit> pph_rec;
	// pcr_pool_amplicons (pcr_pool_amplicons.inc): the records' intervals, their {gc, other, reversed}, the u32 and u64 arrays carved from one buffer
	// each (sort keys and order, run starts, representatives, counts, class tables), the info records, scan / sort scratch, the packed spellings.
	DevBuf<uint4> pam_iv, pam_stat; DevBuf<uint32_t> pam_u32; DevBuf<uint64_t> pam_u64; DevBuf<pcr_amplicon_info> pam_info; DevBuf<uint8_t> pam_tmp, pam_packed;
	uint32_t bg_max_pairs = 0;        // pcr_background_match: the largest batch whose oligo geometry k_bg_emit's workgroup can hold in LDS (0: not asked yet)
	uint32_t amp_dbg_hash_bits = 0;   // PCRAMP_DEBUG_AMP_HASH_BITS=<bits>: pcr_pool_amplicons groups by that many bits of its hash, so that unequal spellings share a key and its resolve path runs (tests)
	// pcr_pool_probe_candidates (pcr_probe_candidates.inc): the records' inserts, the start positions' offsets + chunk counts and offsets + error flag,
	// the u32 and u64 arrays carved from one buffer each (occurrences, sort keys and indices, flags and their scans), the candidate and the kept
	// records, scan / sort scratch.
	DevBuf<uint4> ppc_iv; DevBuf<uint32_t> ppc_pos, ppc_u32; DevBuf<uint64_t> ppc_u64; DevBuf<pcr_probe_candidate> ppc_rec; DevBuf<uint8_t> ppc_tmp;
	// pcr_pool_anneal_profile (pcr_anneal_profile.inc), beside `shared`: the melt rows of the pool's distinct (plus, minus) keys + the spurious row,
	// the histograms and per-temperature sums, pair_sequences.
	DevBuf<uint32_t> anp_pairseq; DevBuf<uint64_t> anp_out; DevBuf<float> anp_melt;
	// pcr_pool_conflicts (pcr_pool_conflicts.inc), beside `shared` (whose flag holds two words here: k_item_tm's, k_pool_dimer_reduce's): attribution
	// offsets, (cell, sequence) keys and melt bits, the cells with a product and their aggregates, the dense aggregates; pcr_pool_dimers' tables,
	// per-duplex results, per-cell records and keep words, the dense tm_max matrix; the cells' records, keep words and their scan, the kept records.
	DevBuf<uint8_t> pcf_din; DevBuf<uint32_t> pcf_vals, pcf_ucell, pcf_dkeep, pcf_keep, pcf_koff;
	DevBuf<uint64_t> pcf_aoff, pcf_keys; DevBuf<float4> pcf_dres;
	DevBuf<uint4> pcf_uagg, pcf_dense; DevBuf<pcr_pool_dimer> pcf_drec; DevBuf<float> pcf_dmat; DevBuf<pcr_pool_conflict> pcf_rec, pcf_out;
	// The one scratch set of pcr_pool_products_tm, pcr_pool_probe_hits, pcr_pool_anneal_profile and pcr_pool_conflicts: each call overwrites what the
	// last one left.  pool_*, site_* and sv_* are apart: they keep their places above, and SvRun hands pointers into site_* / sv_* to pcr_site_repair.
	ItemScratch shared;
	// pcr_pool_products_end3 (pcr_products_end3.inc), beside `shared`: the 3' end of every item's site (an ItemEnd each, kept as uint2: the
	// struct is that file's), the per-item counts before the rule, their sum and its scratch, the pool's bit rows, records, sort keys and order.
	DevBuf<uint2> pe3_end; DevBuf<uint32_t> pe3_before, pe3_ord; DevBuf<uint64_t> pe3_sum, pe3_keys, pe3_bits; DevBuf<uint8_t> pe3_tmp;
	DevBuf<pcr_product_end3> pe3_rec;
	// pcr_pool_dimers_end3 (pcr_pool_dimers_end3.inc), beside pdim_in / pdim_tmp / pdim_flag: the placements per duplex and their scan, the job list,
	// a launch's results, per-cell records and the kept ones, keep flags and their scan (cells, then a launch's jobs), the kept placements.
	DevBuf<uint32_t> pde3_cnt, pde3_off, pde3_keep, pde3_koff; DevBuf<uint2> pde3_jobs; DevBuf<float4> pde3_res;
	DevBuf<pcr_pool_dimer_end3> pde3_rec, pde3_out; DevBuf<pcr_dimer_placement> pde3_place;
	bool pde3_attr_set = false;
	// pcr_pool_conflicts_ext (pcr_pool_conflicts_ext.inc), beside pcf_* and pde3_*: the dense n_ol x n_ol matrix of pcr_pool_dimers_end3's cell
	// records, the cells' 96-byte records and the kept ones.
	DevBuf<pcr_pool_dimer_end3> pcx_dense; DevBuf<pcr_pool_conflict_ext> pcx_rec, pcx_out;
};

namespace {

int drain(pcr_ctx *ctx);
int flush_launcher(pcr_ctx *ctx);
void detach_launcher(pcr_ctx *ctx);
void free_jobs(pcr_ctx *ctx);

// HIP events around the launches of a priced kernel (PCR_PROF_*), on the launch stream, while profiling is on.  The pair is
// handed to the context when the scope ends (also on an error return), so no event is ever left behind.
struct ProfScope {
	pcr_ctx *ctx; int k; Event e0, e1;
	ProfScope(pcr_ctx *c, int kernel, bool on = true) : ctx(c), k(kernel)
	{
		if(!on || !ctx->prof || k < 0 || k >= PCR_PROF_KERNELS) return;
		if(e0.create() != hipSuccess || e1.create() != hipSuccess){ e0.release(); return; }
		(void)hipEventRecord(e0, ctx->stream);
	}
	void finish()
	{
		if(!e0) return;
		(void)hipEventRecord(e1, ctx->stream);
		((k == PCR_PROF_SCAN) ? ctx->prof_events : ctx->prof_events_k[k]).emplace_back(std::move(e0), std::move(e1));
	}
	~ProfScope() { finish(); }
};
// the sets a caller may name (the fourth slot is internal)
constexpr int PCR_SET_SCRATCH = 3;
inline bool set_ok(pcr_set which) { return (unsigned)which <= (unsigned)PCR_SET_MULTIPLEX; }
#define CHECK_SET(which) do{ if(!set_ok(which)){ g_err = "unknown sequence set (PCR_SET_TARGET, PCR_SET_BACKGROUND or PCR_SET_MULTIPLEX)"; return PCR_ERR_ARG; } }while(0)
// First thing in every entry point that touches the handle's device state: wait for the launcher thread to have launched the
// handle's queued passes (flush_launcher, which also brings back a failed pass's error), then look at their counters (drain).
#define FLUSH(ctx) do{ if((ctx)->launcher){ const int frc_ = flush_launcher(ctx); if(frc_ != PCR_OK) return frc_; } }while(0)
#define DRAIN(ctx) do{ FLUSH(ctx); if(!(ctx)->pending.empty()){ const int drc_ = drain(ctx); if(drc_ != PCR_OK) return drc_; } }while(0)

struct HostTimer {
	pcr_ctx *ctx; int slot; std::chrono::steady_clock::time_point t0;
	HostTimer(pcr_ctx *c, int s) : ctx(c), slot(s) { if(ctx->timing) t0 = std::chrono::steady_clock::now(); }
	void next(int s)
	{
		if(!ctx->timing) return;
		const auto t1 = std::chrono::steady_clock::now();
		ctx->t_host[slot] += std::chrono::duration<double, std::micro>(t1 - t0).count();
		slot = s; t0 = t1;
	}
	~HostTimer() { next(slot); }
};

// pcr_split_many: where[2i] = block of the plane store, where[2i+1] = bit of the base in it.  Several splits may share a block.
__global__ void k_apply_splits(const uint64_t *__restrict__ where, uint32_t n, uint32_t *__restrict__ planes /* uint4 per block */, uint32_t *__restrict__ nib)
{
	const uint32_t i = blockIdx.x*blockDim.x + threadIdx.x;
	if(i >= n) return;
	const uint64_t gb = where[2*(size_t)i];
	const uint32_t bit = (uint32_t)where[2*(size_t)i + 1];
	const uint32_t m = ~(1u << bit);
	for(int k = 0;k < 4;++k) atomicAnd(&planes[gb*4 + k], m);
	atomicAnd(&nib[gb*4 + (bit >> 3)], ~(0xFu << ((bit & 7u)*4u)));
}

int upload_irregular(pcr_ctx *ctx, SeqSet &S)
{
	const auto tu0 = std::chrono::steady_clock::now();
	auto ms_since = [&](){ return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tu0).count(); };
	double t_flat = 0, t_sort = 0, t_scan = 0, t_copy1 = 0;
	size_t total = 0;
	for(uint32_t s = 0;s < S.n;++s) total += S.irr_host[s].size();
	std::vector<IrrDev> flat(total);
	std::vector<uint32_t> off(S.n + 1, 0);
	for(int k = 0;k < 256;++k) S.irr_size_count[k] = 0;
	{
		size_t at = 0;
		for(uint32_t s = 0;s < S.n;++s){
			off[s] = (uint32_t)at;
			const std::vector<pcrhost::IrrEntry> &v = S.irr_host[s];
			for(size_t k = 0;k < v.size();++k){
				const pcrhost::IrrEntry &e = v[k];
				IrrDev &d = flat[at++];
				d.w = e.w; d.loc = e.loc; d.seq = s;
				d.meta = (uint32_t)e.strand | ((uint32_t)e.cws << 8) | ((uint32_t)e.ord << 16);
				d.local_id = (uint32_t)k;
				++S.irr_size_count[e.cws & 0xFF];
			}
		}
	}
	off[S.n] = (uint32_t)flat.size();
	S.n_irr = (uint32_t)flat.size();
	t_flat = ms_since();
	// scan order: by size counter, largest first, so that a pass with min_oligo_length m walks a prefix (sequence.cpp:157,239 drop
	// the words whose counter is below m); equal counters keep the list's order.  A counting sort: the list is rebuilt after every
	// accepted assay of a design run (pcr_split_many), and a comparison sort of C2's 1.2e6 words was most of the 280 ms that took.
	std::vector<uint32_t> perm(flat.size());
	t_sort = ms_since();
	int rc;
	{
		// bits of a 32-bit plane to the even positions of a 64-bit word
		auto spread = [](uint64_t v) -> uint64_t {
			v = (v | (v << 16)) & 0x0000FFFF0000FFFFull; v = (v | (v << 8)) & 0x00FF00FF00FF00FFull; v = (v | (v << 4)) & 0x0F0F0F0F0F0F0F0Full;
			v = (v | (v << 2)) & 0x3333333333333333ull; v = (v | (v << 1)) & 0x5555555555555555ull; return v;
		};
		// one pass in list order: a word goes to the next free place of its size counter's run, and its scan record is written there
		// (reads in sequence, writes into a handful of runs that each grow in sequence; gathering the records in scan order
		// instead -- a random 48-byte read per word -- was 48 of the 61 ms this took for C2's 1.2e6 words)
		uint32_t start[256];
		uint32_t run = 0;
		for(int k = 255;k >= 0;--k){ start[k] = run; run += S.irr_size_count[k]; }
		std::vector<IrrScan> scan(perm.size());
		uint32_t n_multi = 0;
		for(size_t i = 0;i < flat.size();++i){
			const IrrDev &d = flat[i];
			const uint32_t at = start[(d.meta >> 8) & 0xFF]++;
			perm[at] = (uint32_t)i;
			const uint32_t multi = (d.w.a & d.w.c) | (d.w.a & d.w.g) | (d.w.a & d.w.t) | (d.w.c & d.w.g) | (d.w.c & d.w.t) | (d.w.g & d.w.t);
			if(multi) ++n_multi;
			const uint32_t lo = d.w.c | d.w.t, hi = d.w.g | d.w.t;             // 2-bit code planes (A,C,G,T = 0..3; empty slots read as A)
			const uint64_t code = spread(lo) | (spread(hi) << 1);
			IrrScan r; r.w0 = (uint32_t)code; r.w1 = (uint32_t)(code >> 32); r.idx_flags = (uint32_t)i | (multi ? 0x80000000u : 0u); r.seq = d.seq;
			scan[at] = r;
		}
		S.irr_n_multi = n_multi; S.irx_valid = false;
		t_scan = ms_since();
		if((rc = S.irr_scan.ensure_slack(scan.size() + 1)) != PCR_OK) return rc;
		if(!scan.empty()) HIP_TRY(hipMemcpy(S.irr_scan.p, scan.data(), scan.size()*sizeof(IrrScan), hipMemcpyHostToDevice));
	}
	t_copy1 = ms_since();
	if((rc = S.irr_perm.ensure_slack(perm.size() + 1)) != PCR_OK) return rc;
	if(!perm.empty()) HIP_TRY(hipMemcpyAsync(S.irr_perm.p, perm.data(), perm.size()*sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
	if((rc = S.irr.ensure_slack(flat.size())) != PCR_OK) return rc;
	if((rc = S.irr_off.ensure(off.size())) != PCR_OK) return rc;
	if(!flat.empty()) HIP_TRY(hipMemcpyAsync(S.irr.p, flat.data(), flat.size()*sizeof(IrrDev), hipMemcpyHostToDevice, ctx->stream));
	HIP_TRY(hipMemcpyAsync(S.irr_off.p, off.data(), off.size()*sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
	HIP_TRY(hipStreamSynchronize(ctx->stream));
	if(ctx->timing && flat.size() > 100000) fprintf(stderr, "[pcramp] irregular list of %zu words: flat %.1f  order %.1f  scan records %.1f  first copy %.1f  other copies %.1f ms\n", flat.size(), t_flat, t_sort - t_flat, t_scan - t_sort, t_copy1 - t_scan, ms_since() - t_copy1);
	return PCR_OK;
}

// starts[] = the exclusive prefix sums of counts[0 .. n), and counts[] = a copy of them; sums: one word per 4096 counts
void launch_exclusive_scan(pcr_ctx *ctx, uint32_t *counts, uint32_t *starts, uint32_t n, uint32_t *sums)
{
	const uint32_t n_blocks = (n + 4095u)/4096u;
	hipLaunchKernelGGL(k_scan_blocks, dim3(n_blocks), dim3(1024), 0, ctx->stream, counts, starts, n, sums);
	hipLaunchKernelGGL(k_scan_sums, dim3(1), dim3(1024), 0, ctx->stream, sums, n_blocks);
	hipLaunchKernelGGL(k_scan_add, dim3(n_blocks), dim3(1024), 0, ctx->stream, starts, counts, n, sums);
}

// The inverse index of the set's irregular words (pcr_scan_seed2.inc), for the state the set is in: counting sort of (word, slot
// offset) by the 9-gram read there.  ~1 ms for C2's 1.2e6 words; rebuilt after the irregular list changes (load, splits).
constexpr uint32_t IRX_MAX_RUN = 1024;
int ensure_irr_index(pcr_ctx *ctx, SeqSet &S)
{
	if(S.irx_valid) return PCR_OK;
	int rc;
	if((rc = S.irx_first.ensure(IRX_KEYS + 4)) != PCR_OK) return rc;
	if((rc = S.irx_last.ensure(IRX_KEYS + 4)) != PCR_OK) return rc;
	if((rc = S.irx_words.ensure_slack((size_t)24*S.n_irr + 4)) != PCR_OK) return rc;
	const uint32_t n_blocks = (IRX_KEYS + 4095u)/4096u;                           // 1 536
	if((rc = S.irx_sums.ensure(n_blocks + 4)) != PCR_OK) return rc;
	HIP_TRY(hipMemsetAsync(S.irx_last.p, 0, (size_t)IRX_KEYS*sizeof(uint32_t), ctx->stream));   // counts first, ends of the runs in the end
	if(S.n_irr){
		hipLaunchKernelGGL(k_irx_count, dim3((S.n_irr + 255)/256), dim3(256), 0, ctx->stream, S.irr.p, S.n_irr, S.irx_last.p);
		HIP_TRY(hipGetLastError());
	}
	{
		// a key shared by more words than a wave should walk (IRX_MAX_RUN): the set keeps the chunk form of the irregular scan
		uint32_t longest = 0;
		HIP_TRY(hipMemsetAsync(S.irx_sums.p + n_blocks, 0, sizeof(uint32_t), ctx->stream));
		hipLaunchKernelGGL(k_irx_max, dim3(256), dim3(256), 0, ctx->stream, S.irx_last.p, IRX_KEYS, S.irx_sums.p + n_blocks);
		HIP_TRY(hipMemcpyAsync(&longest, S.irx_sums.p + n_blocks, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
		HIP_TRY(hipStreamSynchronize(ctx->stream));
		S.irx_usable = longest <= IRX_MAX_RUN;
		if(!S.irx_usable){ S.irx_valid = true; return PCR_OK; }
	}
	launch_exclusive_scan(ctx, S.irx_last.p, S.irx_first.p, IRX_KEYS, S.irx_sums.p);   // first = starts; last = a copy, advanced by the scatter to the ends
	HIP_TRY(hipGetLastError());
	if(S.n_irr){
		hipLaunchKernelGGL(k_irx_scatter, dim3((S.n_irr + 255)/256), dim3(256), 0, ctx->stream, S.irr.p, S.n_irr, S.irx_last.p, S.irx_words.p);
		HIP_TRY(hipGetLastError());
	}
	S.irx_valid = true;
	return PCR_OK;
}

// The set's positions by the 9-gram that starts there and the base behind it (pcr_scan_seed3.inc), each with the 23 + 23 context bases
// around it: counting sort on the device.  One 16-byte entry per base; built once per load.
int ensure_pos_index(pcr_ctx *ctx, SeqSet &S)
{
	if(S.pix_valid) return PCR_OK;
	S.pix_valid = true; S.pix_usable = false;
	if(S.total_blocks == 0 || S.total_blocks*32 >= (uint64_t(1) << 32) - 64) return PCR_OK;   // positions are 32-bit
	int rc;
	if((rc = S.pix_first.ensure(PIX_KEYS + 4)) != PCR_OK) return rc;
	if((rc = S.pix_last.ensure(PIX_KEYS + 4)) != PCR_OK) return rc;
	const uint32_t n_blocks = (PIX_KEYS + 4095u)/4096u;
	if((rc = S.pix_sums.ensure(n_blocks + 4)) != PCR_OK) return rc;
	if((rc = S.pix_ent.ensure(S.total_blocks*32 + 64)) != PCR_OK) return rc;
	{
		// per 32-base block: its sequence (bit 31: the tile it lies in holds IUPAC codes) and its number within the sequence -- what a
		// window that reached its floor is asked, in one round trip
		if(S.n >= (1u << 30)){ return PCR_OK; }
		if((rc = S.blk_info.ensure(S.total_blocks + 1)) != PCR_OK) return rc;
		if((rc = S.blk_local.ensure(S.total_blocks + 1)) != PCR_OK) return rc;
		// (made on the device: a C4 shard has 10^8 blocks)
		std::vector<uint32_t> tile0((size_t)S.n + 1);
		uint64_t t0 = 0;
		for(uint32_t q = 0;q < S.n;++q){ tile0[q] = (uint32_t)t0; t0 += (S.len[q] >= 32) ? (S.len[q] - 7 + TILE_POS - 1)/TILE_POS : 0; }
		tile0[S.n] = (uint32_t)t0;
		if(t0 >= (uint64_t(1) << 32)) return PCR_OK;
		if((rc = S.blk_tile0.ensure((size_t)S.n + 1)) != PCR_OK) return rc;
		HIP_TRY(hipMemcpyAsync(S.blk_tile0.p, tile0.data(), ((size_t)S.n + 1)*sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
		hipLaunchKernelGGL(k_blk_info, dim3((unsigned)((S.total_blocks + 255)/256)), dim3(256), 0, ctx->stream, S.blk_seq.p, S.d_blk_off.p, S.d_len.p,
			S.blk_tile0.p, S.tile_degen.p, S.d_active.p, S.total_blocks, S.blk_info.p, S.blk_local.p);
		HIP_TRY(hipGetLastError());
		HIP_TRY(hipStreamSynchronize(ctx->stream));                                  // (tile0 is a local)
	}
	HIP_TRY(hipMemsetAsync(S.pix_last.p, 0, (size_t)PIX_KEYS*sizeof(uint32_t), ctx->stream));
	const unsigned grid = (unsigned)((S.total_blocks + 255)/256);
	hipLaunchKernelGGL(k_pix_build<false>, dim3(grid), dim3(256), 0, ctx->stream, S.tb_d(), S.blk_seq.p, S.d_blk_off.p, S.d_len.p, S.total_blocks, S.pix_last.p, (uint4 *)nullptr);
	launch_exclusive_scan(ctx, S.pix_last.p, S.pix_first.p, PIX_KEYS, S.pix_sums.p);
	hipLaunchKernelGGL(k_pix_build<true>, dim3(grid), dim3(256), 0, ctx->stream, S.tb_d(), S.blk_seq.p, S.d_blk_off.p, S.d_len.p, S.total_blocks, S.pix_last.p, S.pix_ent.p);
	HIP_TRY(hipGetLastError());
	{
		// the host's mirror: the exclusive prefix of the PIX_KEYS sub-run lengths and their total -- a span's length is one subtraction
		S.pix_start_h.resize((size_t)PIX_KEYS + 1);
		HIP_TRY(hipMemcpyAsync(S.pix_start_h.data(), S.pix_first.p, (size_t)PIX_KEYS*sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
		HIP_TRY(hipMemcpyAsync(S.pix_start_h.data() + PIX_KEYS, S.pix_last.p + (PIX_KEYS - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
		HIP_TRY(hipStreamSynchronize(ctx->stream));
		static uint64_t generations = 0;
		S.pix_generation = ++generations;
	}
	S.pix_usable = true;
	return PCR_OK;
}

int run_valid(pcr_ctx *ctx, SeqSet &S, uint64_t first_block, uint64_t n_blocks)
{
	if(n_blocks == 0) return PCR_OK;
	const unsigned threads = 256;
	const unsigned grid = (unsigned)((n_blocks + threads - 1)/threads);
	hipLaunchKernelGGL(k_valid, dim3(grid), dim3(threads), 0, ctx->stream, S.planes.p, S.d_blk_off.p, S.blk_seq.p,
		S.d_nblk_real.p, S.valid_d(), S.total_blocks, ctx->filt.max_degen, ctx->filt.gc_ok, first_block, n_blocks);
	HIP_TRY(hipGetLastError());
	return PCR_OK;
}

int build_tile_desc(pcr_ctx *ctx, SeqSet &S)
{
	if(S.n_tiles == 0) return PCR_OK;
	int rc = S.tile_desc.ensure(S.n_tiles);
	if(rc != PCR_OK) return rc;
	hipLaunchKernelGGL(k_tile_desc, dim3((S.n_tiles + 255)/256), dim3(256), 0, ctx->stream, S.d_blk_off.p, S.d_len.p, S.d_active.p, S.tile_seq.p,
		S.tile_pos0.p, S.tile_degen.p, S.n_tiles, S.tile_desc.p);
	HIP_TRY(hipGetLastError());
	return PCR_OK;
}

void fill_oligo_planes(OligoDev &o, const Planes &m, float thr2)
{
	o.m = m;
	const unsigned size = (unsigned)pcrhost::planes_size(o.m);
	o.floor2 = (unsigned)((float)size*thr2);                                     // optimize.cpp:293
	o.norm = (size > 0) ? (float)(1.0/size) : 0.0f;                              // optimize.cpp:221
	o.start = pcrhost::planes_start(o.m);
	o.stop = pcrhost::planes_stop(o.m);
	o.p1 = (o.stop >= 1) ? pcrhost::planes_nibble(o.m, o.stop - 1) : 0;
	o.p2 = (o.stop >= 0) ? pcrhost::planes_nibble(o.m, o.stop) : 0;
}

void fill_oligo(OligoDev &o, const uint64_t w[2], float thr2) { fill_oligo_planes(o, pcrhost::planes_of_word(w), thr2); }

// Packs small host arrays into a host-mapped pinned buffer; ONE kernel (k_stage) pulls them into the
// device arena and clears up to two device regions in the same launch -- a copy-engine transfer and a
// fill each cost ~4 us plus a ~6 us queue bubble on either side, a kernel runs back to back with the next.
__global__ void k_stage(const uint4 *__restrict__ src, uint4 *__restrict__ dst, uint32_t n16,
	uint4 *__restrict__ z0, uint32_t n0, uint4 *__restrict__ z1, uint32_t n1, uint4 *__restrict__ z2, uint32_t n2)
{
	const uint32_t i = blockIdx.x*blockDim.x + threadIdx.x, stride = gridDim.x*blockDim.x;
	for(uint32_t k = i;k < n16;k += stride) dst[k] = src[k];
	const uint4 zero = make_uint4(0, 0, 0, 0);
	for(uint32_t k = i;k < n0;k += stride) z0[k] = zero;
	for(uint32_t k = i;k < n1;k += stride) z1[k] = zero;
	for(uint32_t k = i;k < n2;k += stride) z2[k] = zero;
}

// Spins until seen() holds -- a flag in host-mapped memory that a kernel of `stream` raises -- and asks the stream every
// 16 384 spins whether anything is still running on it.  On SPIN_ERROR, err holds the stream's error.
enum SpinEnd { SPIN_SEEN, SPIN_IDLE, SPIN_ERROR };
template<class Seen> inline SpinEnd spin_until(hipStream_t stream, Seen seen, hipError_t &err)
{
	for(uint64_t spins = 1;!seen();++spins){
		__builtin_ia32_pause();
		if((spins & 0x3FFF) == 0){
			err = hipStreamQuery(stream);
			if(err == hipSuccess) return SPIN_IDLE;
			if(err != hipErrorNotReady) return SPIN_ERROR;
		}
	}
	return SPIN_SEEN;
}

// Has the pass with mailbox sequence number `seq` published?  Publications happen in stream order and slot
// seq % MAIL_RING is reused by seq + MAIL_RING, ...: any value of that slot at or beyond seq means yes.
int wait_published(pcr_ctx *ctx, uint32_t seq)
{
	const PassMail *const slot = ctx->mail.host + (seq % pcr_ctx::MAIL_RING);
	hipError_t e = hipSuccess;
	const SpinEnd end = spin_until(ctx->stream, [&]{
		const uint32_t v = __atomic_load_n((const uint32_t *)&slot->seq, __ATOMIC_ACQUIRE);
		return v >= seq && (v - seq) % pcr_ctx::MAIL_RING == 0; }, e);
	if(end == SPIN_ERROR){ g_err = std::string("device pass failed: ") + hipGetErrorString(e); return PCR_ERR_DEVICE; }
	return PCR_OK;                                              // (stream idle: whatever used the slot is over; the pass may have failed before publishing)
}

struct Stager {
	pcr_ctx *ctx; size_t used = 0; bool direct = false;
	explicit Stager(pcr_ctx *c) : ctx(c) {}
	pcr_ctx::StageSlot *slot = nullptr; pcr_ctx::DirectSlot *dslot = nullptr;   // the slot of this call, in stage[] or (direct) in dstage[]
	uint8_t *host = nullptr, *dev = nullptr;                     // the slot's bytes as the CPU and as the kernels address them
	// direct: the bytes go straight into a slot of device memory (see pcr_ctx::dstage); the caller launches no k_stage for
	// them and passes the sequence number of ITS pass to seal(): the slot is free again once the NEXT pass has published,
	// i.e. once every kernel of this one is over.
	int begin_direct(size_t bytes)
	{
		direct = true;
		dslot = &ctx->dstage[ctx->dstage_next];
		ctx->dstage_next = (ctx->dstage_next + 1) % pcr_ctx::STAGE_RING;
		if(dslot->guard_seq){ const int grc = wait_published(ctx, dslot->guard_seq); if(grc != PCR_OK) return grc; dslot->guard_seq = 0; }
		if(bytes + 256 > dslot->buf.cap){
			if(dslot->buf.p) HIP_TRY(hipStreamSynchronize(ctx->stream));
			const int rc = dslot->buf.ensure(std::max<size_t>((bytes + 256)*2, 1 << 17));
			if(rc != PCR_OK) return rc;
		}
		host = dev = dslot->buf.p;                                  // one address for the CPU's stores and the kernels' loads
		used = 0;
		return PCR_OK;
	}
	void seal(uint32_t pass_seq)
	{
		__builtin_ia32_sfence();                                     // the write-combined stores leave the core before the doorbell is rung
		dslot->guard_seq = pass_seq + 1;
	}
	int begin(size_t bytes)
	{
		slot = &ctx->stage[ctx->stage_next];
		ctx->stage_next = (ctx->stage_next + 1) % pcr_ctx::STAGE_RING;
		if(slot->busy){ HIP_TRY(hipEventSynchronize(slot->done)); slot->busy = false; }
		if(slot->guard_seq){ const int grc = wait_published(ctx, slot->guard_seq); if(grc != PCR_OK) return grc; slot->guard_seq = 0; }
		int rc = slot->buf.ensure(bytes, std::max<size_t>(bytes*2, 1 << 16));
		if(rc != PCR_OK) return rc;
		host = slot->buf.host; dev = slot->buf.dev;
		if(!slot->done) HIP_TRY(slot->done.create(hipEventDisableTiming));
		rc = ctx->arena.ensure(bytes + 256);
		used = 0;
		return rc;
	}
	// returns the DEVICE address the bytes will have
	template<class T> T *put(const T *src, size_t n)
	{
		used = (used + 15) & ~size_t(15);
		memcpy(host + used, src, n*sizeof(T));
		T *at = (T *)((direct ? dev : ctx->arena.p) + used);
		used += n*sizeof(T);
		return at;
	}
	// z0/z1: device regions to clear in the same launch (16-byte aligned, sizes rounded UP to 16 bytes: the
	// caller's buffers must be allocated with that slack)
	int ship(void *z0 = nullptr, size_t bytes0 = 0, void *z1 = nullptr, size_t bytes1 = 0, void *z2 = nullptr, size_t bytes2 = 0, uint32_t guard_seq = 0)
	{
		const uint32_t n16 = (uint32_t)((used + 15)/16), n0 = (uint32_t)((bytes0 + 15)/16), n1 = (uint32_t)((bytes1 + 15)/16), n2 = (uint32_t)((bytes2 + 15)/16);
		const uint32_t most = std::max(std::max(n16, n2), std::max(n0, n1));
		if(most){
			const unsigned grid = std::min<unsigned>((most + 255)/256, 512u);
			hipLaunchKernelGGL(k_stage, dim3(grid), dim3(256), 0, ctx->stream, (const uint4 *)dev, (uint4 *)ctx->arena.p, n16,
				(uint4 *)z0, n0, (uint4 *)z1, n1, (uint4 *)z2, n2);
			HIP_TRY(hipGetLastError());
		}
		// The slot may be rewritten once k_stage has run.  A pass publishes its counters after that (mailbox), so
		// its sequence number is the guard; other callers record an event (an event packet between two kernels
		// costs a ~5 us queue bubble, which is why passes avoid it).
		if(guard_seq) slot->guard_seq = guard_seq;
		else{
			HIP_TRY(hipEventRecord(slot->done, ctx->stream));
			slot->busy = true;
		}
		return PCR_OK;
	}
};

// The pass's counters go to the host through mapped memory: no copy-engine packet, no interrupt wake-up.
__global__ void k_publish(const uint32_t *__restrict__ counters, pcr_ctx::Mail *mail, uint32_t seq)
{
	if(threadIdx.x < 4) mail->counters[threadIdx.x] = counters[threadIdx.x];
	__threadfence_system();
	__syncthreads();
	if(threadIdx.x == 0) __hip_atomic_store((uint32_t *)&mail->seq, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

int mail_wait(pcr_ctx *ctx, uint32_t seq, uint32_t out[4])
{
	pcr_ctx::Mail *const slot = ctx->mail.host + (seq % pcr_ctx::MAIL_RING);
	auto seen = [&]{ return __atomic_load_n((const uint32_t *)&slot->seq, __ATOMIC_ACQUIRE) == seq; };
	hipError_t e = hipSuccess;
	const SpinEnd end = spin_until(ctx->stream, seen, e);
	if(end == SPIN_ERROR){ g_err = std::string("device pass failed: ") + hipGetErrorString(e); return PCR_ERR_DEVICE; }
	if(end == SPIN_IDLE && !seen()){ g_err = "device pass finished without publishing its counters"; return PCR_ERR_DEVICE; }   // everything drained: the flag must be there now
	for(int i = 0;i < 4;++i) out[i] = slot->counters[i];
	return PCR_OK;
}

// ---- small results back to the host through mapped memory (see pcr_ctx::ret_host)
__global__ void k_return(const uint4 *__restrict__ s0, uint32_t n0, const uint4 *__restrict__ s1, uint32_t n1,
	const uint4 *__restrict__ s2, uint32_t n2, uint4 *__restrict__ dst)
{
	const uint32_t stride = gridDim.x*blockDim.x, t = blockIdx.x*blockDim.x + threadIdx.x;
	for(uint32_t i = t;i < n0;i += stride) dst[i] = s0[i];
	for(uint32_t i = t;i < n1;i += stride) dst[n0 + i] = s1[i];
	for(uint32_t i = t;i < n2;i += stride) dst[n0 + n1 + i] = s2[i];
}

__global__ void k_return_flag(uint32_t *flag, uint32_t seq)
{
	__threadfence_system();
	__hip_atomic_store(flag, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// Copies up to three device regions (16-byte aligned; sizes are rounded UP to 16 bytes, so the buffers need that
// slack) back to back into the mapped return buffer and waits for them.  out[k] = host address of region k.
int return_to_host(pcr_ctx *ctx, const void *s0, size_t b0, const void *s1, size_t b1, const void *s2, size_t b2, const uint8_t *out[3])
{
	const uint32_t n0 = (uint32_t)((b0 + 15)/16), n1 = (uint32_t)((b1 + 15)/16), n2 = (uint32_t)((b2 + 15)/16);
	const size_t need = ((size_t)n0 + n1 + n2)*16;
	int rc;
	if(!ctx->ret_flag.host){
		if((rc = ctx->ret_flag.ensure(64)) != PCR_OK) return rc;
		*ctx->ret_flag.host = 0;
	}
	if(need > ctx->ret.cap){
		HIP_TRY(hipStreamSynchronize(ctx->stream));
		if((rc = ctx->ret.ensure(need, std::max<size_t>(need*2, 1 << 20))) != PCR_OK) return rc;
	}
	const uint32_t most = std::max(n0, std::max(n1, n2));
	if(most){
		const unsigned grid = std::min<unsigned>((most + 255)/256, 1024u);
		hipLaunchKernelGGL(k_return, dim3(grid), dim3(256), 0, ctx->stream, (const uint4 *)s0, n0, (const uint4 *)s1, n1, (const uint4 *)s2, n2, (uint4 *)ctx->ret.dev);
		HIP_TRY(hipGetLastError());
	}
	const uint32_t seq = ++ctx->ret_seq;
	hipLaunchKernelGGL(k_return_flag, dim3(1), dim3(1), 0, ctx->stream, ctx->ret_flag.dev, seq);
	HIP_TRY(hipGetLastError());
	auto seen = [&]{ return __atomic_load_n((const uint32_t *)ctx->ret_flag.host, __ATOMIC_ACQUIRE) == seq; };
	hipError_t e = hipSuccess;
	const SpinEnd end = spin_until(ctx->stream, seen, e);
	if(end == SPIN_ERROR){ g_err = std::string("device work failed: ") + hipGetErrorString(e); return PCR_ERR_DEVICE; }
	if(end == SPIN_IDLE && !seen()){ g_err = "device work finished without raising the return flag"; return PCR_ERR_DEVICE; }
	out[0] = ctx->ret.host; out[1] = ctx->ret.host + (size_t)n0*16; out[2] = ctx->ret.host + ((size_t)n0 + n1)*16;
	return PCR_OK;
}

// Small inputs of a synchronous call: copied into a host-mapped buffer that the kernel reads in place (a pageable
// hipMemcpyAsync costs ~20 us).  Valid until the next call; the caller waits for its results before returning.
int mapped_input(pcr_ctx *ctx, const void *src, size_t bytes, const void **dev_out)
{
	if(bytes > ctx->in.cap){
		HIP_TRY(hipStreamSynchronize(ctx->stream));
		const int rc = ctx->in.ensure(bytes, std::max<size_t>(bytes*2, 1 << 18));
		if(rc != PCR_OK) return rc;
	}
	memcpy(ctx->in.host, src, bytes);
	*dev_out = ctx->in.dev;
	return PCR_OK;
}

// pcr_screen_device: the amplicon screen's oligo table and the clearing of its result bitsets ride in the
// select pass's staging launch, and the pass's counters are published by k_match instead of k_publish.
struct FusedAmp {
	const pcr_pair *pairs; uint32_t n_pairs; const pcr_amplify_args *a; uint64_t *d_fr, *d_rf;
	bool staged = false; const OligoDev *d_oligos = nullptr; uint32_t pub_seq = 0; const uint32_t *pub_counters = nullptr;
	bool posted = false;       // k_post ran the whole tail (amplicon screen included)
};

void build_oligos(const pcr_pair *pairs, uint32_t n_pairs, const pcr_amplify_args *a, std::vector<OligoDev> &ol)
{
	const float thr2 = a->collect_threshold*a->collect_threshold;                // pcr_assay.cpp:31-32
	ol.resize(2*(size_t)n_pairs);
	for(uint32_t i = 0;i < n_pairs;++i){
		fill_oligo(ol[2*i], pairs[i].f.w, thr2);
		fill_oligo(ol[2*i + 1], pairs[i].r.w, thr2);
	}
}

// The fused tail (k_post) leaves the DB in place but builds no touched list: do it for the callers that walk it.
int ensure_touched(pcr_ctx *ctx, SeqSet &S)
{
	if(S.touched_built || !S.have_db || !S.ctrl.p) return PCR_OK;
	if(S.touched_from_seg) hipLaunchKernelGGL(k_touched_seg, dim3((S.n + 255)/256), dim3(256), 0, ctx->stream, S.d_seg_hi, S.n, S.ctrl.p, S.touched.p);
	else hipLaunchKernelGGL(k_touched, dim3((S.n + 255)/256), dim3(256), 0, ctx->stream, S.ctrl.p + 8, S.n, S.ctrl.p, S.touched.p);
	HIP_TRY(hipGetLastError());
	uint32_t n = 0;
	HIP_TRY(hipMemcpyAsync(&n, S.ctrl.p + 3, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
	HIP_TRY(hipStreamSynchronize(ctx->stream));
	S.n_touched = n; S.n_entries = n ? 1 : 0; S.touched_built = true;
	return PCR_OK;
}

int amplify_launch(pcr_ctx *ctx, SeqSet &S, const pcr_pair *pairs, uint32_t n_pairs, const pcr_amplify_args *a,
	uint64_t *d_fr, uint64_t *d_rf, const FusedAmp *fa = nullptr)
{
	{ const int erc = ensure_touched(ctx, S); if(erc != PCR_OK) return erc; }
	if(!S.have_db){ g_err = "pcr_amplify: no word DB (call pcr_select_words first)"; return PCR_ERR_STATE; }
	const uint64_t words = (S.n + 63)/64;
	const size_t bits_bytes = (size_t)n_pairs*words*sizeof(uint64_t);
	if(S.n_entries == 0 || n_pairs == 0){
		if(bits_bytes){
			HIP_TRY(hipMemsetAsync(d_fr, 0, bits_bytes, ctx->stream));
			HIP_TRY(hipMemsetAsync(d_rf, 0, bits_bytes, ctx->stream));
		}
		return PCR_OK;
	}
	HostTimer timer(ctx, 4);
	int rc;
	const bool prestaged = fa && fa->staged;
	if(prestaged) ctx->d_oligos = fa->d_oligos;
	else{
		std::vector<OligoDev> ol;
		build_oligos(pairs, n_pairs, a, ol);
		Stager st(ctx);
		if((rc = st.begin(ol.size()*sizeof(OligoDev) + 64)) != PCR_OK) return rc;
		ctx->d_oligos = st.put(ol.data(), ol.size());
		// the result bitsets are cleared by the staging kernel when they allow 16-byte stores
		const bool vec_ok = ((uintptr_t)d_fr % 16 == 0) && ((uintptr_t)d_rf % 16 == 0) && (bits_bytes % 16 == 0);
		if(!vec_ok){
			HIP_TRY(hipMemsetAsync(d_fr, 0, bits_bytes, ctx->stream));
			HIP_TRY(hipMemsetAsync(d_rf, 0, bits_bytes, ctx->stream));
		}
		if((rc = vec_ok ? st.ship(d_fr, bits_bytes, d_rf, bits_bytes) : st.ship()) != PCR_OK) return rc;
	}
	timer.next(5);
	const uint32_t mask_words = (2*n_pairs + 31)/32;
	if((rc = ctx->mask.ensure((size_t)S.n_slots*mask_words)) != PCR_OK) return rc;
	if((rc = ctx->status.ensure(1)) != PCR_OK) return rc;
	// the number of touched sequences: known to the host after a synchronous select, read on the device
	// (conservative grids, grid-stride loops) after an asynchronous one
	const bool dev_n = S.n_touched == N_TOUCHED_UNKNOWN;
	const uint32_t *n_dev = dev_n ? S.ctrl.p + 3 : nullptr;
	const uint32_t n_t = dev_n ? 0u : S.n_touched, n_db = n_t*S.db_cap;
	const unsigned threads = dev_n ? 256 : 128;
	const unsigned grid = dev_n ? (unsigned)std::min<uint64_t>(((uint64_t)S.n*S.db_cap + threads - 1)/threads, 1024) : (n_db + threads - 1)/threads;
	const unsigned mgrid = dev_n ? std::min<unsigned>((S.n + MATCH_WAVES - 1)/MATCH_WAVES, 1024u) : (n_t + MATCH_WAVES - 1)/MATCH_WAVES;
	// k_match also clears the status word (it runs before k_pair in stream order)
	hipLaunchKernelGGL(k_match, dim3(std::max(mgrid, 1u)), dim3(64*MATCH_WAVES), 0, ctx->stream, S.db.p, n_t, n_dev, S.db_cap,
		S.touched.p, S.d_seg_hi, ctx->d_oligos, 2*n_pairs, mask_words, ctx->mask.p, ctx->status.p,
		prestaged ? fa->pub_counters : (const uint32_t *)nullptr, prestaged ? ctx->mail.dev + (fa->pub_seq % pcr_ctx::MAIL_RING) : (pcr_ctx::Mail *)nullptr,
		prestaged ? fa->pub_seq : 0u);
	HIP_TRY(hipGetLastError());
	hipLaunchKernelGGL(k_pair, dim3(grid), dim3(threads), 0, ctx->stream, S.db.p, n_db, n_dev, S.db_cap, S.touched.p, S.d_seg_hi, ctx->mask.p,
		mask_words, ctx->d_oligos, n_pairs, S.planes.p, S.d_blk_off.p, S.d_len.p, S.d_active.p, a->amp_min, a->amp_max,
		a->ident_threshold, a->use_taq_mama, d_fr, d_rf, words, ctx->status.p);
	HIP_TRY(hipGetLastError());
	return PCR_OK;
}

template<int NSLOT, int KLO>
int launch_scan2_nw(pcr_ctx *ctx, SeqSet &S, uint32_t nw, uint32_t group0, uint32_t n_groups, uint32_t gw, uint32_t ncand, const HitSink &sink,
	const uint32_t *d_tab, const uint32_t *d_bias, const uint32_t *tile_ids, uint32_t n_tiles, const uint32_t *orient_ids)
{
#define SCAN2_ARGS S.nib.p, S.planes.p, S.valid_d(), S.d_blk_off.p, S.d_len.p, S.d_active.p, S.tile_seq.p, S.tile_pos0.p, \
	d_tab, d_bias, group0, gw, tile_ids, orient_ids, ctx->d_cand_fwd, ctx->d_cand_rc, ctx->d_cand_floor, ncand, sink
	const dim3 grid(n_tiles, n_groups), block(SCAN2_THREADS);
	switch(nw){
		case 1: hipLaunchKernelGGL((k_scan2<1, NSLOT, KLO>), grid, block, 0, ctx->stream, SCAN2_ARGS); break;
		case 2: hipLaunchKernelGGL((k_scan2<2, NSLOT, KLO>), grid, block, 0, ctx->stream, SCAN2_ARGS); break;
		case 3: hipLaunchKernelGGL((k_scan2<3, NSLOT, KLO>), grid, block, 0, ctx->stream, SCAN2_ARGS); break;
		case 4: hipLaunchKernelGGL((k_scan2<4, NSLOT, KLO>), grid, block, 0, ctx->stream, SCAN2_ARGS); break;
		case 5: hipLaunchKernelGGL((k_scan2<5, NSLOT, KLO>), grid, block, 0, ctx->stream, SCAN2_ARGS); break;
		case 6: hipLaunchKernelGGL((k_scan2<6, NSLOT, KLO>), grid, block, 0, ctx->stream, SCAN2_ARGS); break;
		case 7: hipLaunchKernelGGL((k_scan2<7, NSLOT, KLO>), grid, block, 0, ctx->stream, SCAN2_ARGS); break;
		default: hipLaunchKernelGGL((k_scan2<8, NSLOT, KLO>), grid, block, 0, ctx->stream, SCAN2_ARGS); break;
	}
#undef SCAN2_ARGS
	HIP_TRY(hipGetLastError());
	return PCR_OK;
}

// The bit-sliced scan over all orientation groups: full groups (8 words) in one launch, the
// partial last group in a second one.
int launch_scan2(pcr_ctx *ctx, SeqSet &S, const Scan2Tables &T, uint32_t ncand, const HitSink &sink,
	const uint32_t *d_tab, const uint32_t *d_bias, const uint32_t *tile_ids, uint32_t n_tiles, const uint32_t *orient_ids)
{
	if(n_tiles == 0 || T.n_groups == 0) return PCR_OK;
	const uint32_t full = (T.last_words == T.gw) ? T.n_groups : T.n_groups - 1;
	int rc = PCR_OK;
	if(full){
		rc = (T.nslot == 26) ? launch_scan2_nw<26, 3>(ctx, S, T.gw, 0, full, T.gw, ncand, sink, d_tab, d_bias, tile_ids, n_tiles, orient_ids)
			: launch_scan2_nw<32, 0>(ctx, S, T.gw, 0, full, T.gw, ncand, sink, d_tab, d_bias, tile_ids, n_tiles, orient_ids);
		if(rc != PCR_OK) return rc;
	}
	if(full < T.n_groups){
		rc = (T.nslot == 26) ? launch_scan2_nw<26, 3>(ctx, S, T.last_words, full, 1, T.gw, ncand, sink, d_tab, d_bias, tile_ids, n_tiles, orient_ids)
			: launch_scan2_nw<32, 0>(ctx, S, T.last_words, full, 1, T.gw, ncand, sink, d_tab, d_bias, tile_ids, n_tiles, orient_ids);
	}
	return rc;
}

// Exact DB size: sum of the per-sequence fills (done on the host on request; a device-side
// same-address atomic per sequence would serialise, ~35 ns each).
int count_entries(pcr_ctx *ctx, SeqSet &S)
{
	uint64_t total = 0;
	if(S.n_touched){
		std::vector<uint32_t> hi(S.n);
		HIP_TRY(hipMemcpyAsync(hi.data(), S.d_seg_hi, S.n*sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
		HIP_TRY(hipStreamSynchronize(ctx->stream));
		for(uint32_t q = 0;q < S.n;++q){ if(hi[q]) total += hi[q] - (uint64_t)q*S.db_cap; }
	}
	S.n_entries = (uint32_t)total;
	return PCR_OK;
}

} // namespace

// ============================================================================== C-ABI
extern "C" {

const char *pcr_last_error(void) { return g_err.c_str(); }

pcr_ctx *pcr_create(int device, void *hip_stream, const pcr_params *params)
{
	int count = 0;
	if(hipGetDeviceCount(&count) != hipSuccess || count <= 0){
		g_err = "pcr_create: no HIP device available (this library has no CPU fallback)";
		return nullptr;
	}
	if(device < 0 || device >= count){ g_err = "pcr_create: bad device index"; return nullptr; }
	if(hipSetDevice(device) != hipSuccess){ g_err = "pcr_create: hipSetDevice failed"; return nullptr; }
	hipDeviceProp_t prop;
	if(hipGetDeviceProperties(&prop, device) != hipSuccess){ g_err = "pcr_create: hipGetDeviceProperties failed"; return nullptr; }
	if(std::string(prop.gcnArchName).find("gfx950") == std::string::npos){
		g_err = std::string("pcr_create: device is ") + prop.gcnArchName + ", this build targets gfx950 only";
		return nullptr;
	}
	pcr_ctx *ctx = new pcr_ctx();
	ctx->device = device;
	if(hip_stream) ctx->stream.borrow((hipStream_t)hip_stream);
	else if(ctx->stream.create() != hipSuccess){ g_err = "pcr_create: hipStreamCreate failed"; delete ctx; return nullptr; }
	if(params){ ctx->params = *params; }
	else{ ctx->params.pack_max_degen = 256; ctx->params.pack_min_gc = 0.0f; ctx->params.pack_max_gc = 1.0f; }
	{ hipDeviceProp_t prop; if(hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) ctx->n_cu = (uint32_t)prop.multiProcessorCount; }
	if(const char *v = getenv("PCRAMP_TIMING")) ctx->timing = v[0] == '1';
	ctx->debug_log = getenv("PCRAMP_DEBUG") != nullptr;
	if(const char *v = getenv("PCRAMP_DEBUG_EPOCH")) ctx->debug_epoch = (uint32_t)strtoul(v, nullptr, 0);   // test hook: start the pass counter near its wrap
	if(const char *v = getenv("PCRAMP_OPT_PM")) ctx->opt_pm_global = v[0] == 'g';
	if(const char *v = getenv("PCRAMP_DEBUG_OPT_TASKS")){ unsigned a = 0, b = 0; if(sscanf(v, "%u,%u", &a, &b) >= 1){ ctx->opt_dbg_wg_tasks = a; ctx->opt_dbg_task_cap = b; } }
	if(const char *v = getenv("PCRAMP_DEBUG_AMP_HASH_BITS")) ctx->amp_dbg_hash_bits = (uint32_t)strtoul(v, nullptr, 0);
	if(const char *v = getenv("PCRAMP_DEBUG_AMP_CAP")) ctx->amp_cap = std::max<size_t>(16, (size_t)strtoull(v, nullptr, 0));   // test hook: a small candidate amplicon list, so that its overflow and the repeated pass run (at least one record per sub-list)
	if(const char *v = getenv("PCRAMP_SEED")) ctx->force_seed1 = v[0] == '1';
	if(const char *v = getenv("PCRAMP_SEED_TABLES")) ctx->host_seed_tables = v[0] == 'h';
	if(const char *v = getenv("PCRAMP_S2DBG")) ctx->s2_dbg = (uint32_t)atoi(v);
	if(const char *v = getenv("PCRAMP_IRR_INDEX")) ctx->no_irr_index = v[0] == '0';
	if(const char *v = getenv("PCRAMP_SEED3")) ctx->no_seed3 = v[0] == '0';
	if(const char *v = getenv("PCRAMP_S3_NEXT")) ctx->s3_next = v[0] != '0';
	if(const char *v = getenv("PCRAMP_SEED_MEMO")) ctx->seed_lists.use_memo = v[0] != '0';
	if(const char *v = getenv("PCRAMP_LAUNCH_THREAD")) ctx->launch_thread = v[0] != '0';   // A/B, and for callers that want no helper thread
	if(const char *v = getenv("PCRAMP_PAIR")) ctx->pair_mode = (v[0] == '0') ? 0 : (strcmp(v, "force") == 0) ? 2 : 1;
	if(const char *v = getenv("PCRAMP_SCAN")){ if(v[0] == '1') ctx->scan_version = 1; else if(v[0] == '2') ctx->scan_version = 2; }   // A/B: 1 = popcount scan, 2 = bit-sliced only
	{
		// direct staging: fine-grained device memory the CPU can store into (large BAR) and whose stores a later launch sees.
		// Probed, not assumed: the device must report a large BAR (otherwise a CPU store into the allocation would fault), and a
		// pattern stored by the CPU, fenced, must come back through a kernel that copies it into mapped host memory.
		const char *v = getenv("PCRAMP_STAGE");
		if(!(v && v[0] == 'k') && prop.isLargeBar){
			DevBuf<uint32_t> probe(true); MappedBuf<uint32_t> back; const std::string err_before = g_err;
			constexpr uint32_t PROBE_WORDS = 1024;
			if(probe.ensure(PROBE_WORDS) == PCR_OK && back.ensure(PROBE_WORDS*sizeof(uint32_t)) == PCR_OK){
				hipPointerAttribute_t at;
				bool ok = hipPointerGetAttributes(&at, probe.p) == hipSuccess;
				for(int round = 0;ok && round < 2;++round){
					volatile uint32_t *w = (volatile uint32_t *)probe.p;
					for(uint32_t i = 0;i < PROBE_WORDS;++i){ w[i] = 0x9E3779B9u*(i + 1) + (uint32_t)round; back.host[i] = 0; }
					__builtin_ia32_sfence();
					hipLaunchKernelGGL(k_stage, dim3(1), dim3(256), 0, ctx->stream, (const uint4 *)probe.p, (uint4 *)back.dev, PROBE_WORDS/4,
						(uint4 *)nullptr, 0u, (uint4 *)nullptr, 0u, (uint4 *)nullptr, 0u);
					ok = hipGetLastError() == hipSuccess && hipStreamSynchronize(ctx->stream) == hipSuccess;
					for(uint32_t i = 0;ok && i < PROBE_WORDS;++i) ok = back.host[i] == 0x9E3779B9u*(i + 1) + (uint32_t)round;
				}
				ctx->direct_ok = ok;
			}
			else{ (void)hipGetLastError(); g_err = err_before; }    // (no large-BAR staging: not an error of pcr_create)
		}
	}
	ctx->filt.max_degen = ctx->params.pack_max_degen;
	ctx->filt.set_gc(ctx->params.pack_min_gc, ctx->params.pack_max_gc);
	if(hipMemcpyToSymbol(HIP_SYMBOL(c_taq_mama), h_taq_mama, sizeof(h_taq_mama)) != hipSuccess ||
	   hipMemcpyToSymbol(HIP_SYMBOL(thermo::c_H), PCR_NN_H, sizeof(PCR_NN_H)) != hipSuccess ||
	   hipMemcpyToSymbol(HIP_SYMBOL(thermo::c_S), PCR_NN_S, sizeof(PCR_NN_S)) != hipSuccess ||
	   hipMemcpyToSymbol(HIP_SYMBOL(thermo::c_loop_S), PCR_LOOP_S, sizeof(PCR_LOOP_S)) != hipSuccess ||
	   hipMemcpyToSymbol(HIP_SYMBOL(thermo::c_bulge_S), PCR_BULGE_S, sizeof(PCR_BULGE_S)) != hipSuccess ||
	   hipMemcpyToSymbol(HIP_SYMBOL(thermo::c_hairpin_S), PCR_HAIRPIN_S, sizeof(PCR_HAIRPIN_S)) != hipSuccess ||
	   hipMemcpyToSymbol(HIP_SYMBOL(thermo::c_special_H), PCR_SPECIAL_H, sizeof(PCR_SPECIAL_H)) != hipSuccess ||
	   hipMemcpyToSymbol(HIP_SYMBOL(thermo::c_special_S), PCR_SPECIAL_S, sizeof(PCR_SPECIAL_S)) != hipSuccess ||
	   hipMemcpyToSymbol(HIP_SYMBOL(thermo::c_special_key), PCR_SPECIAL_KEY, sizeof(PCR_SPECIAL_KEY)) != hipSuccess ||
	   hipMemcpyToSymbol(HIP_SYMBOL(thermo::c_wc), PCR_WC, sizeof(PCR_WC)) != hipSuccess){
		g_err = "pcr_create: hipMemcpyToSymbol failed"; delete ctx; return nullptr;
	}
	if(ctx->mail.ensure(sizeof(pcr_ctx::Mail)*pcr_ctx::MAIL_RING) != PCR_OK){ g_err = "pcr_create: mapped host allocation failed"; delete ctx; return nullptr; }
	memset((void *)ctx->mail.host, 0, sizeof(pcr_ctx::Mail)*pcr_ctx::MAIL_RING);
	return ctx;
}

void pcr_destroy(pcr_ctx *ctx)
{
	if(!ctx) return;
	(void)hipSetDevice(ctx->device);
	(void)flush_launcher(ctx);                    // queued passes are launched (or dropped after a failed one) before anything is freed
	detach_launcher(ctx);                         // the stream's last handle stops and joins the launcher thread
	(void)hipStreamSynchronize(ctx->stream);      // nothing may be in flight when the owners free (pcr_owned.hpp): synchronise, then delete
	if(ctx->aux_stream) (void)hipStreamSynchronize(ctx->aux_stream);
	ctx->pending.clear();
	free_jobs(ctx);
	if(ctx->timing && ctx->n_timed){
		const double n = (double)ctx->n_timed;
		fprintf(stderr, "[pcramp] host us/pass by stage: A (plan, caller's thread) %.1f  B (stage + launch, %s) %.1f  (%llu of %llu passes pipelined, queue depth <= %u)\n",
			ctx->t_host[0]/n, ctx->n_pipelined ? "launcher thread" : "caller's thread", (ctx->t_host[1] + ctx->t_host[2])/n,
			(unsigned long long)ctx->n_pipelined, (unsigned long long)ctx->n_timed, ctx->lq_client.max_depth);
		fprintf(stderr, "[pcramp] host us/pass: plan %.1f  stage %.1f  launch %.1f  wait %.1f | amplify prep %.1f  launch %.1f  (%llu passes)\n",
			ctx->t_host[0]/n, ctx->t_host[1]/n, ctx->t_host[2]/n, ctx->t_host[3]/n, ctx->t_host[4]/n, ctx->t_host[5]/n, (unsigned long long)ctx->n_timed);
	}
	delete ctx;
}

uint32_t pcr_num_sequences(pcr_ctx *ctx, pcr_set which) { return (ctx && set_ok(which)) ? ctx->sets[which].n : 0; }
uint64_t pcr_bitset_words(pcr_ctx *ctx, pcr_set which) { return (ctx && set_ok(which)) ? (ctx->sets[which].n + 63)/64 : 0; }

int pcr_staging_mode(pcr_ctx *ctx) { return (ctx && ctx->direct_ok) ? 1 : 0; }

int pcr_launcher_stats(pcr_ctx *ctx, uint64_t *passes_pipelined, uint32_t *max_queue_depth)
{
	if(!ctx){ g_err = "null ctx"; return PCR_ERR_ARG; }
	if(passes_pipelined) *passes_pipelined = ctx->n_pipelined;
	if(max_queue_depth) *max_queue_depth = ctx->lq_client.max_depth;
	return PCR_OK;
}

int pcr_live_resources(uint64_t out[4])
{
	if(!out){ g_err = "pcr_live_resources: bad argument"; return PCR_ERR_ARG; }
	for(int k = 0;k < 4;++k) out[k] = pcrown::g_live[k].load();
	return PCR_OK;
}

int pcr_synchronize(pcr_ctx *ctx)
{
	if(!ctx){ g_err = "null ctx"; return PCR_ERR_ARG; }
	HIP_TRY(hipSetDevice(ctx->device));
	DRAIN(ctx);
	HIP_TRY(hipStreamSynchronize(ctx->stream));
	return PCR_OK;
}

static int load_sequences_impl(pcr_ctx *ctx, int which, const uint8_t *packed4, const uint64_t *byte_offsets,
	const uint64_t *lengths, const float *weights, uint32_t n);

int pcr_load_sequences(pcr_ctx *ctx, pcr_set which, const uint8_t *packed4, const uint64_t *byte_offsets,
	const uint64_t *lengths, const float *weights, uint32_t n)
{
	if(!set_ok(which)){ g_err = "pcr_load_sequences: unknown sequence set"; return PCR_ERR_ARG; }
	return load_sequences_impl(ctx, (int)which, packed4, byte_offsets, lengths, weights, n);
}

// (which may be the internal scratch set)
static int load_sequences_impl(pcr_ctx *ctx, int which, const uint8_t *packed4, const uint64_t *byte_offsets,
	const uint64_t *lengths, const float *weights, uint32_t n)
{
	if(!ctx || which < 0 || which >= PCR_N_SETS || (n && (!packed4 || !byte_offsets || !lengths))){
		g_err = "pcr_load_sequences: bad argument"; return PCR_ERR_ARG;
	}
	DRAIN(ctx);
	if(n >= (1u << 24)){ g_err = "pcr_load_sequences: at most 2^24-1 sequences per GPU shard"; return PCR_ERR_CAPACITY; }
	HIP_TRY(hipSetDevice(ctx->device));
	// a pass publishes its mailbox before its last kernel has finished (k_post publishes at its start): the blocking
	// copies below go through the null stream, which a caller-supplied non-blocking stream does not order against
	HIP_TRY(hipStreamSynchronize(ctx->stream));
	SeqSet &S = ctx->sets[which];
	S.have_db = false; S.n_entries = 0; S.have_codes = false;
	S.n = n;
	S.packed.assign(n, std::vector<uint8_t>());
	S.len.assign(lengths, lengths + n);
	if(which == PCR_SET_TARGET) ctx->drop_shard();                                  // a new target set is not the shard that was attached
	if(which == PCR_SET_TARGET || which == PCR_SET_BACKGROUND) ctx->trial_comm = nullptr;   // nor are new sets the ones the ranks agreed on
	S.weight.assign(n, 1.0f);
	if(weights) S.weight.assign(weights, weights + n);
	S.weight_dirty = true;
	S.ctrl_clean = false; S.touched_from_seg = false;
	S.active.assign(n, 1);
	S.has_eos.assign(n, 0);
	S.blk_off.assign(n + 1, 0);
	S.nblk_real.assign(n, 0);
	S.irr_host.assign(n, std::vector<pcrhost::IrrEntry>());
	uint64_t total_bytes = 0, total_blocks = 0, n_tiles = 0;
	std::vector<uint64_t> dev_byte_off(n);
	for(uint32_t s = 0;s < n;++s){
		if(lengths[s] >= (uint64_t(1) << 31)){ g_err = "pcr_load_sequences: sequence longer than 2^31-1 bases"; return PCR_ERR_CAPACITY; }
		const uint64_t nb = (lengths[s] + 1)/2;
		S.packed[s].assign(packed4 + byte_offsets[s], packed4 + byte_offsets[s] + nb);
		if((lengths[s] & 1) && nb) S.packed[s][nb - 1] &= 0xF0;                  // pad nibble = EOS (sequence.cpp:21)
		{
			const std::vector<uint8_t> &b = S.packed[s];
			bool eos = false;
			const uint64_t full = lengths[s]/2;
			for(uint64_t k = 0;k < full && !eos;++k) eos = ((b[k] & 0xF0) == 0) || ((b[k] & 0x0F) == 0);
			if(!eos && (lengths[s] & 1)) eos = ((b[full] & 0xF0) == 0);
			S.has_eos[s] = eos ? 1 : 0;
		}
		dev_byte_off[s] = total_bytes;
		total_bytes += nb;
		S.blk_off[s] = total_blocks;
		S.nblk_real[s] = (lengths[s] + 31)/32;
		total_blocks += S.nblk_real[s] + 2;
		if(lengths[s] >= 32) n_tiles += (lengths[s] - 7 + TILE_POS - 1)/TILE_POS;   // tiles cover window starts 0..L-32 AND seed positions 0..L-8 (k_seed)
	}
	S.blk_off[n] = total_blocks;
	S.total_blocks = total_blocks;
	if(n_tiles >= (uint64_t(1) << 31)){ g_err = "pcr_load_sequences: too many tiles"; return PCR_ERR_CAPACITY; }
	S.n_tiles = (uint32_t)n_tiles;

	// host-side index pieces: block -> sequence map, tile list, irregular words
	std::vector<uint32_t> blk_seq(total_blocks), tile_seq(n_tiles), tile_pos0(n_tiles);
	uint64_t t = 0;
	S.pix_valid = false; S.pix_usable = false;
	for(uint32_t s = 0;s < n;++s){
		for(uint64_t b = S.blk_off[s];b < S.blk_off[s + 1];++b) blk_seq[b] = s;
		if(lengths[s] >= 32){
			const uint64_t nt = (lengths[s] - 7 + TILE_POS - 1)/TILE_POS;
			for(uint64_t k = 0;k < nt;++k, ++t){ tile_seq[t] = s; tile_pos0[t] = (uint32_t)(k*TILE_POS); }
		}
		pcrhost::PackedSeq q; q.buf = S.packed[s].data(); q.len = lengths[s];
		if(!pcrhost::irregular_words(q, ctx->filt, S.irr_host[s])){
			g_err = "pcr_load_sequences: more than 64 irregular words share one (loc, strand)"; return PCR_ERR_CAPACITY;
		}
	}

	int rc;
	DevBuf<uint8_t> d_packed; DevBuf<uint64_t> d_byte_off;
	if((rc = d_packed.ensure(total_bytes)) != PCR_OK) return rc;
	if((rc = d_byte_off.ensure(n)) != PCR_OK) return rc;
	if((rc = S.planes.ensure(total_blocks)) != PCR_OK) return rc;
	if((rc = S.valid.ensure(S2_VALID_FRONT + total_blocks + S2_TAIL_BLOCKS)) != PCR_OK) return rc;
	if((rc = S.nib.ensure(total_blocks*4 + 8)) != PCR_OK) return rc;
	if((rc = S.tb.ensure(S2_TB_FRONT + (total_blocks + S2_TAIL_BLOCKS)*2 + 8)) != PCR_OK) return rc;
	if((rc = S.tile_degen.ensure(n_tiles + 1)) != PCR_OK) return rc;
	if((rc = S.degen_tiles.ensure(n_tiles + 1)) != PCR_OK) return rc;
	if((rc = S.blk_seq.ensure(total_blocks)) != PCR_OK) return rc;
	if((rc = S.tile_seq.ensure(n_tiles)) != PCR_OK) return rc;
	if((rc = S.tile_pos0.ensure(n_tiles)) != PCR_OK) return rc;
	if((rc = S.d_len.ensure(n)) != PCR_OK) return rc;
	if((rc = S.d_blk_off.ensure(n + 1)) != PCR_OK) return rc;
	if((rc = S.d_nblk_real.ensure(n)) != PCR_OK) return rc;
	if((rc = S.d_active.ensure(n)) != PCR_OK) return rc;
	if((rc = S.d_has_eos.ensure(n)) != PCR_OK) return rc;
#define H2D(dst, src, bytes) do{ if((bytes) > 0){ hipError_t e_ = hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice); \
	if(e_ != hipSuccess){ g_err = std::string("hipMemcpy: ") + hipGetErrorString(e_); return PCR_ERR_DEVICE; } } }while(0)
	{   // one transfer for all sequences (a copy per sequence was 10 000 copy-engine packets at C2)
		std::vector<uint8_t> flat(total_bytes);
		for(uint32_t s = 0;s < n;++s){ if(!S.packed[s].empty()) memcpy(flat.data() + dev_byte_off[s], S.packed[s].data(), S.packed[s].size()); }
		H2D(d_packed.p, flat.data(), flat.size());
	}
	H2D(d_byte_off.p, dev_byte_off.data(), n*sizeof(uint64_t));
	H2D(S.blk_seq.p, blk_seq.data(), total_blocks*sizeof(uint32_t));
	H2D(S.tile_seq.p, tile_seq.data(), n_tiles*sizeof(uint32_t));
	H2D(S.tile_pos0.p, tile_pos0.data(), n_tiles*sizeof(uint32_t));
	H2D(S.d_len.p, S.len.data(), n*sizeof(uint64_t));
	H2D(S.d_blk_off.p, S.blk_off.data(), (n + 1)*sizeof(uint64_t));
	H2D(S.d_nblk_real.p, S.nblk_real.data(), n*sizeof(uint64_t));
	H2D(S.d_active.p, S.active.data(), n);
	H2D(S.d_has_eos.p, S.has_eos.data(), n);
#undef H2D
	{   // the padding in front of and behind valid[] / tb[] (what k_seed2's unchecked tile fetch may touch beyond the sequences)
		hipError_t e_ = hipMemsetAsync(S.valid.p, 0, S2_VALID_FRONT*sizeof(uint32_t), ctx->stream);
		if(e_ == hipSuccess) e_ = hipMemsetAsync(S.valid_d() + total_blocks, 0, S2_TAIL_BLOCKS*sizeof(uint32_t), ctx->stream);
		if(e_ == hipSuccess) e_ = hipMemsetAsync(S.tb.p, 0, S2_TB_FRONT*sizeof(uint32_t), ctx->stream);
		if(e_ == hipSuccess) e_ = hipMemsetAsync(S.tb_d() + total_blocks*2, 0, (S2_TAIL_BLOCKS*2 + 8)*sizeof(uint32_t), ctx->stream);
		if(e_ != hipSuccess){ g_err = std::string("load: padding memset: ") + hipGetErrorString(e_); return PCR_ERR_DEVICE; }
	}
	if(total_blocks){
		const unsigned threads = 256;
		const unsigned grid = (unsigned)((total_blocks + threads - 1)/threads);
		hipLaunchKernelGGL(k_transpose, dim3(grid), dim3(threads), 0, ctx->stream, d_packed.p, d_byte_off.p, S.d_len.p,
			S.d_blk_off.p, S.blk_seq.p, S.planes.p, S.nib.p, S.tb_d(), total_blocks);
		if(hipGetLastError() != hipSuccess){ g_err = "k_transpose launch failed"; return PCR_ERR_DEVICE; }
		if((rc = run_valid(ctx, S, 0, total_blocks)) != PCR_OK) return rc;
	}
	S.bucket_cap = 64;               // grown by earlier passes over other data: start small again
	S.n_degen_tiles = 0;
	if(n_tiles){
		hipLaunchKernelGGL(k_tile_degen, dim3((unsigned)((n_tiles + 255)/256)), dim3(256), 0, ctx->stream, S.planes.p, S.d_blk_off.p,
			S.d_nblk_real.p, S.tile_seq.p, S.tile_pos0.p, (uint32_t)n_tiles, S.tile_degen.p);
		if(hipGetLastError() != hipSuccess){ g_err = "k_tile_degen launch failed"; return PCR_ERR_DEVICE; }
	}
	if(total_blocks >= (uint64_t(1) << 40)){ g_err = "pcr_load_sequences: more than 2^40 blocks"; return PCR_ERR_CAPACITY; }
	if((rc = build_tile_desc(ctx, S)) != PCR_OK) return rc;
	if(hipStreamSynchronize(ctx->stream) != hipSuccess){ g_err = "load: stream sync failed"; return PCR_ERR_DEVICE; }
	if(n_tiles){
		std::vector<uint8_t> flags(n_tiles);
		std::vector<uint32_t> list;
		if(hipMemcpy(flags.data(), S.tile_degen.p, n_tiles, hipMemcpyDeviceToHost) != hipSuccess){ g_err = "load: flag download failed"; return PCR_ERR_DEVICE; }
		for(uint64_t t2 = 0;t2 < n_tiles;++t2){ if(flags[t2]) list.push_back((uint32_t)t2); }
		S.n_degen_tiles = (uint32_t)list.size();
		if(!list.empty() && hipMemcpy(S.degen_tiles.p, list.data(), list.size()*sizeof(uint32_t), hipMemcpyHostToDevice) != hipSuccess){
			g_err = "load: tile list upload failed"; return PCR_ERR_DEVICE;
		}
	}
	d_packed.release(); d_byte_off.release();     // (before the irregular lists are allocated: the packed copy is as large as the set)
	return upload_irregular(ctx, S);
}

int pcr_set_active(pcr_ctx *ctx, pcr_set which, const uint8_t *active)
{
	if(!set_ok(which)){ g_err = "pcr_set_active: unknown sequence set"; return PCR_ERR_ARG; }
	if(!ctx || !active){ g_err = "pcr_set_active: bad argument"; return PCR_ERR_ARG; }
	DRAIN(ctx);
	HIP_TRY(hipSetDevice(ctx->device));
	SeqSet &S = ctx->sets[which];
	for(uint32_t i = 0;i < S.n;++i) S.active[i] = active[i] ? 1 : 0;
	if(S.n){
		HIP_TRY(hipMemcpyAsync(S.d_active.p, S.active.data(), S.n, hipMemcpyHostToDevice, ctx->stream));
		{ const int rc = build_tile_desc(ctx, S); if(rc != PCR_OK) return rc; }
		if(S.pix_valid && S.pix_usable && S.total_blocks){                       // the third form reads the flag out of its per-block words
			hipLaunchKernelGGL(k_blk_active, dim3((unsigned)((S.total_blocks + 255)/256)), dim3(256), 0, ctx->stream, S.blk_info.p, S.blk_seq.p, S.d_active.p, S.total_blocks);
			HIP_TRY(hipGetLastError());
		}
		HIP_TRY(hipStreamSynchronize(ctx->stream));
	}
	return PCR_OK;
}

int pcr_split_many(pcr_ctx *ctx, pcr_set which, const uint32_t *seq, const uint64_t *pos, uint32_t n)
{
	if(!set_ok(which)){ g_err = "pcr_split: unknown sequence set"; return PCR_ERR_ARG; }
	if(!ctx || (n && (!seq || !pos))){ g_err = "pcr_split: bad argument"; return PCR_ERR_ARG; }
	if(n == 0) return PCR_OK;
	DRAIN(ctx);
	HIP_TRY(hipSetDevice(ctx->device));
	SeqSet &S = ctx->sets[which];
	for(uint32_t i = 0;i < n;++i){ if(seq[i] >= S.n || pos[i] >= S.len[seq[i]]){ g_err = "pcr_split: out of range"; return PCR_ERR_ARG; } }
	// host copy, and what the device has to change: per split the block of the plane store and the base's bit in it
	std::vector<uint64_t> where(2*(size_t)n);
	std::vector<uint32_t> touched_seq;
	bool eos_changed = false;
	for(uint32_t i = 0;i < n;++i){
		uint8_t &v = S.packed[seq[i]][pos[i] >> 1];
		v = (pos[i] & 1) ? (v & 0xF0) : (v & 0x0F);                                // sequence.h:232-241
		if(!S.has_eos[seq[i]]){ S.has_eos[seq[i]] = 1; eos_changed = true; }
		where[2*(size_t)i] = S.blk_off[seq[i]] + (pos[i] >> 5); where[2*(size_t)i + 1] = pos[i] & 31u;
		touched_seq.push_back(seq[i]);
	}
	std::sort(touched_seq.begin(), touched_seq.end());
	touched_seq.erase(std::unique(touched_seq.begin(), touched_seq.end()), touched_seq.end());
	int rc;
	if(eos_changed) HIP_TRY(hipMemcpyAsync(S.d_has_eos.p, S.has_eos.data(), S.n, hipMemcpyHostToDevice, ctx->stream));
	// device: clear the bases in their blocks (one launch), refresh the 2 blocks of windows that can see each, redo the irregular
	// lists of the sequences concerned and upload the set's list ONCE (it is rebuilt whole: order by size counter, scan records --
	// tens of ms for C2's 1.2e6 words, which every one of a design iteration's ~70 splits paid when this took one split per call)
	if((rc = ctx->split_where.ensure(where.size())) != PCR_OK) return rc;
	HIP_TRY(hipMemcpyAsync(ctx->split_where.p, where.data(), where.size()*sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
	hipLaunchKernelGGL(k_apply_splits, dim3((n + 255)/256), dim3(256), 0, ctx->stream, ctx->split_where.p, n, (uint32_t *)S.planes.p, S.nib.p);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipStreamSynchronize(ctx->stream));                                   // `where` is a local
	for(uint32_t i = 0;i < n;++i){
		const uint64_t gb = where[2*(size_t)i];
		const uint64_t first = (gb > S.blk_off[seq[i]]) ? gb - 1 : gb;
		if((rc = run_valid(ctx, S, first, gb - first + 1)) != PCR_OK) return rc;
	}
	const auto t0 = std::chrono::steady_clock::now();
	for(uint32_t sq : touched_seq){
		S.irr_host[sq].clear();
		pcrhost::PackedSeq q; q.buf = S.packed[sq].data(); q.len = S.len[sq];
		if(!pcrhost::irregular_words(q, ctx->filt, S.irr_host[sq])){ g_err = "pcr_split: irregular word overflow"; return PCR_ERR_CAPACITY; }
	}
	S.have_db = false; S.have_codes = false;
	const auto t1 = std::chrono::steady_clock::now();
	rc = upload_irregular(ctx, S);
	if(ctx->timing) fprintf(stderr, "[pcramp] split_many: %u splits in %zu sequences; irregular words %.1f ms, list upload %.1f ms\n", n, touched_seq.size(),
		std::chrono::duration<double, std::milli>(t1 - t0).count(), std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count());
	return rc;
}

int pcr_split(pcr_ctx *ctx, pcr_set which, uint32_t seq, uint64_t pos)
{
	return pcr_split_many(ctx, which, &seq, &pos, 1);
}

} // extern "C"

#include "pcr_select.inc"
#include "pcr_select_sites.inc"

extern "C" {

int pcr_select_words(pcr_ctx *ctx, pcr_set which, const pcr_pair *pairs, uint32_t n_pairs, int optimize_5, int optimize_3,
	float threshold, uint32_t min_oligo_length, uint64_t *n_entries_out)
{
	if(!set_ok(which)){ g_err = "pcr_select_words: unknown sequence set"; return PCR_ERR_ARG; }
	if(!ctx || (n_pairs && !pairs)){ g_err = "pcr_select_words: bad argument"; return PCR_ERR_ARG; }
	DRAIN(ctx);
	return select_impl(ctx, which, pairs, n_pairs, optimize_5, optimize_3, threshold, min_oligo_length, n_entries_out, false);
}

int pcr_screen_device(pcr_ctx *ctx, pcr_set which, const pcr_pair *pairs, uint32_t n_pairs, int optimize_5, int optimize_3,
	float select_threshold, uint32_t min_oligo_length, const pcr_amplify_args *args, uint64_t *d_bits_fr, uint64_t *d_bits_rf)
{
	if(!set_ok(which)){ g_err = "pcr_screen_device: unknown sequence set"; return PCR_ERR_ARG; }
	if(!ctx || !args || (n_pairs && (!pairs || !d_bits_fr || !d_bits_rf))){ g_err = "pcr_screen_device: bad argument"; return PCR_ERR_ARG; }
	if(ctx->pending.size() + 2 >= pcr_ctx::MAIL_RING) DRAIN(ctx);     // the mailbox ring bounds how far the host may run ahead
	return screen_pass(ctx, which, pairs, n_pairs, optimize_5, optimize_3, select_threshold, min_oligo_length, args, d_bits_fr, d_bits_rf);
}

int64_t pcr_get_entries(pcr_ctx *ctx, pcr_set which, pcr_entry *out, uint64_t cap)
{
	if(!set_ok(which)){ g_err = "pcr_get_entries: unknown sequence set"; return PCR_ERR_ARG; }
	if(!ctx){ g_err = "null ctx"; return PCR_ERR_ARG; }
	DRAIN(ctx);
	SeqSet &S = ctx->sets[which];
	if(!S.have_db){ g_err = "pcr_get_entries: no word DB"; return PCR_ERR_STATE; }
	{ const int rc = count_entries(ctx, S); if(rc != PCR_OK) return rc; }
	if(cap && out && S.n_entries){
		std::vector<DevEntry> h(S.n_slots);
		std::vector<uint32_t> hi(S.n);
		hipError_t e = hipStreamSynchronize(ctx->stream);
		if(e == hipSuccess) e = hipMemcpy(h.data(), S.db.p, S.n_slots*sizeof(DevEntry), hipMemcpyDeviceToHost);
		if(e == hipSuccess) e = hipMemcpy(hi.data(), S.d_seg_hi, S.n*sizeof(uint32_t), hipMemcpyDeviceToHost);
		if(e != hipSuccess){ g_err = std::string("pcr_get_entries: ") + hipGetErrorString(e); return PCR_ERR_DEVICE; }
		uint64_t k = 0;
		for(uint32_t q = 0;q < S.n && k < cap;++q){
			for(uint32_t i = q*S.db_cap;i < hi[q] && k < cap;++i, ++k){
				pcrhost::word_of_planes(h[i].w, out[k].word.w);
				out[k].loc = h[i].loc; out[k].index = h[i].seq; out[k].strand = h[i].strand; out[k].pad = 0;
			}
		}
	}
	return (int64_t)S.n_entries;
}

int pcr_amplify_device(pcr_ctx *ctx, pcr_set which, const pcr_pair *pairs, uint32_t n_pairs, const pcr_amplify_args *args,
	uint64_t *d_bits_fr, uint64_t *d_bits_rf)
{
	if(!set_ok(which)){ g_err = "pcr_amplify_device: unknown sequence set"; return PCR_ERR_ARG; }
	if(!ctx || !args || (n_pairs && (!pairs || !d_bits_fr || !d_bits_rf))){ g_err = "pcr_amplify_device: bad argument"; return PCR_ERR_ARG; }
	DRAIN(ctx);
	HIP_TRY(hipSetDevice(ctx->device));
	return amplify_launch(ctx, ctx->sets[which], pairs, n_pairs, args, d_bits_fr, d_bits_rf);
}

int pcr_amplify(pcr_ctx *ctx, pcr_set which, const pcr_pair *pairs, uint32_t n_pairs, const pcr_amplify_args *args,
	uint64_t *bits, uint64_t *bits_fr, uint64_t *bits_rf, float *coverage)
{
	if(!set_ok(which)){ g_err = "pcr_amplify: unknown sequence set"; return PCR_ERR_ARG; }
	if(!ctx || !args || (n_pairs && !pairs)){ g_err = "pcr_amplify: bad argument"; return PCR_ERR_ARG; }
	DRAIN(ctx);
	HIP_TRY(hipSetDevice(ctx->device));
	SeqSet &S = ctx->sets[which];
	const uint64_t words = (S.n + 63)/64;
	const size_t total = (size_t)n_pairs*words;
	int rc;
	if((rc = ctx->bits_fr.ensure(total + 2)) != PCR_OK) return rc;               // + 2: return_to_host copies whole 16-byte units
	if((rc = ctx->bits_rf.ensure(total + 2)) != PCR_OK) return rc;
	if((rc = ctx->status.ensure(1)) != PCR_OK) return rc;
	if((rc = amplify_launch(ctx, S, pairs, n_pairs, args, ctx->bits_fr.p, ctx->bits_rf.p)) != PCR_OK) return rc;
	const bool have_status = S.n_entries && n_pairs;                             // the screen ran and wrote the status word
	const uint8_t *back[3];
	if((rc = return_to_host(ctx, ctx->bits_fr.p, total*sizeof(uint64_t), ctx->bits_rf.p, total*sizeof(uint64_t),
		have_status ? ctx->status.p : nullptr, have_status ? sizeof(uint32_t) : 0, back)) != PCR_OK) return rc;
	const uint64_t *hfr = (const uint64_t *)back[0], *hrf = (const uint64_t *)back[1];
	const uint32_t status = have_status ? *(const uint32_t *)back[2] : 0u;
	if(status & 1u){ g_err = "Sequence::has_split: range is out of bounds"; return PCR_ERR_RANGE; }   // sequence.cpp:306-308
	for(uint32_t p = 0;p < n_pairs;++p){
		if(bits){ for(uint64_t w = 0;w < words;++w) bits[p*words + w] = hfr[p*words + w] | hrf[p*words + w]; }
		if(bits_fr) memcpy(bits_fr + p*words, hfr + p*words, words*sizeof(uint64_t));
		if(bits_rf) memcpy(bits_rf + p*words, hrf + p*words, words*sizeof(uint64_t));
		if(coverage) coverage[p] = pcr_coverage_from_bits(hfr + p*words, hrf + p*words, S.weight.data(), S.n);
	}
	return PCR_OK;
}

int pcr_move_coverage(pcr_ctx *ctx, pcr_set which, const pcr_pair *base, int side, const pcr_word128 *variants, uint32_t n_variants,
	const pcr_amplify_args *args, uint64_t *bits_fr, uint64_t *bits_rf, float *coverage)
{
	if(!set_ok(which)){ g_err = "pcr_move_coverage: unknown sequence set"; return PCR_ERR_ARG; }
	if(!ctx || !args || !base || (side != 0 && side != 1) || (n_variants && !variants)){ g_err = "pcr_move_coverage: bad argument"; return PCR_ERR_ARG; }
	DRAIN(ctx);
	HIP_TRY(hipSetDevice(ctx->device));
	SeqSet &S = ctx->sets[which];
	if(!S.have_db){ g_err = "pcr_move_coverage: no word DB (call pcr_select_words first)"; return PCR_ERR_STATE; }
	{ const int erc = ensure_touched(ctx, S); if(erc != PCR_OK) return erc; }
	const uint64_t words = (S.n + 63)/64;
	const size_t total = (size_t)n_variants*words;
	if(coverage){ for(uint32_t v = 0;v < n_variants;++v) coverage[v] = 0.0f; }
	if(bits_fr && total) memset(bits_fr, 0, total*sizeof(uint64_t));
	if(bits_rf && total) memset(bits_rf, 0, total*sizeof(uint64_t));
	if(S.n_entries == 0 || n_variants == 0) return PCR_OK;
	int rc;
	// oligo table: base F, base R (floors from the collect threshold, pcr_assay.cpp:31-32), then the variants
	const float thr2 = args->collect_threshold*args->collect_threshold;
	std::vector<OligoDev> ol(2 + (size_t)n_variants);
	fill_oligo(ol[0], base->f.w, thr2);
	fill_oligo(ol[1], base->r.w, thr2);
	for(uint32_t v = 0;v < n_variants;++v){
		if((variants[v].w[0] | variants[v].w[1]) == 0){ g_err = "pcr_move_coverage: empty trial oligo"; return PCR_ERR_ARG; }
		fill_oligo(ol[2 + v], variants[v].w, thr2);
	}
	if((rc = ctx->bits_fr.ensure(total + 2)) != PCR_OK) return rc;
	if((rc = ctx->bits_rf.ensure(total + 2)) != PCR_OK) return rc;
	Stager st(ctx);
	if((rc = st.begin(ol.size()*sizeof(OligoDev) + 64)) != PCR_OK) return rc;
	const OligoDev *d_ol = st.put(ol.data(), ol.size());
	if((rc = st.ship(ctx->bits_fr.p, total*sizeof(uint64_t), ctx->bits_rf.p, total*sizeof(uint64_t))) != PCR_OK) return rc;
	if((rc = ctx->mask.ensure((size_t)S.n_slots)) != PCR_OK) return rc;
	if((rc = ctx->status.ensure(1)) != PCR_OK) return rc;
	const uint32_t n_db = S.n_touched*S.db_cap;
	hipLaunchKernelGGL(k_match_few, dim3((n_db + 255)/256), dim3(256), 0, ctx->stream, S.db.p, n_db, S.db_cap, S.touched.p, S.d_seg_hi, d_ol, 2u,
		ctx->mask.p, ctx->status.p);
	HIP_TRY(hipGetLastError());
	if(S.db_cap >= 256 && S.db_cap <= PMS_MAX)                                    // big buckets: a workgroup per sequence over a compact partner list
		hipLaunchKernelGGL(k_pair_moves_seq, dim3(S.n_touched), dim3(PMS_THREADS), 0, ctx->stream, S.db.p, S.db_cap, S.touched.p, S.d_seg_hi, ctx->mask.p,
			d_ol, d_ol + 2, n_variants, side, S.planes.p, S.d_blk_off.p, S.d_len.p, S.d_active.p, S.d_has_eos.p, args->amp_min, args->amp_max,
			args->ident_threshold, args->use_taq_mama, ctx->bits_fr.p, ctx->bits_rf.p, words, ctx->status.p);
	else
		hipLaunchKernelGGL(k_pair_moves, dim3((n_db + 127)/128), dim3(128), 0, ctx->stream, S.db.p, n_db, S.db_cap, S.touched.p, S.d_seg_hi, ctx->mask.p,
			d_ol, d_ol + 2, n_variants, side, S.planes.p, S.d_blk_off.p, S.d_len.p, S.d_active.p, S.d_has_eos.p, args->amp_min, args->amp_max,
			args->ident_threshold, args->use_taq_mama, ctx->bits_fr.p, ctx->bits_rf.p, words, ctx->status.p);
	HIP_TRY(hipGetLastError());
	const uint8_t *back[3];
	if((rc = return_to_host(ctx, ctx->bits_fr.p, total*sizeof(uint64_t), ctx->bits_rf.p, total*sizeof(uint64_t), ctx->status.p, sizeof(uint32_t), back)) != PCR_OK) return rc;
	const uint64_t *hfr = (const uint64_t *)back[0], *hrf = (const uint64_t *)back[1];
	const uint32_t status = *(const uint32_t *)back[2];
	if(status & 1u){ g_err = "Sequence::has_split: range is out of bounds"; return PCR_ERR_RANGE; }   // sequence.cpp:306-308
	if(bits_fr) memcpy(bits_fr, hfr, total*sizeof(uint64_t));
	if(bits_rf) memcpy(bits_rf, hrf, total*sizeof(uint64_t));
	if(coverage){ for(uint32_t v = 0;v < n_variants;++v) coverage[v] = pcr_coverage_from_bits(hfr + v*words, hrf + v*words, S.weight.data(), S.n); }
	return PCR_OK;
}

float pcr_coverage_from_bits(const uint64_t *bits_fr, const uint64_t *bits_rf, const float *weights, uint64_t n)
{
	// PCR::compute_coverage (pcr_assay.cpp:271-302): amplicons are visited {F(+),R(-)} first in
	// ascending sequence order, then {R(+),F(-)}; each sequence's weight is added once, in double.
	double ret = 0.0;
	const uint64_t nw = (n + 63)/64;
	for(uint64_t w = 0;w < nw;++w){                                               // set bits in ascending order
		for(uint64_t m = bits_fr[w];m;m &= m - 1){ const uint64_t i = w*64 + (uint64_t)__builtin_ctzll(m); if(i < n) ret += weights[i]; }
	}
	for(uint64_t w = 0;w < nw;++w){
		for(uint64_t m = bits_rf[w] & ~bits_fr[w];m;m &= m - 1){ const uint64_t i = w*64 + (uint64_t)__builtin_ctzll(m); if(i < n) ret += weights[i]; }
	}
	return (float)ret;
}

float pcr_weighted_coverage(const uint64_t *bits, const float *weights, uint64_t n)
{
	double ret = 0.0;                                                            // main.cpp:1402-1418
	const uint64_t nw = (n + 63)/64;
	for(uint64_t w = 0;w < nw;++w){
		for(uint64_t m = bits[w];m;m &= m - 1){ const uint64_t i = w*64 + (uint64_t)__builtin_ctzll(m); if(i < n) ret += weights[i]; }
	}
	return (float)ret;
}

int pcr_profile_enable(pcr_ctx *ctx, int on)
{
	if(!ctx){ g_err = "null ctx"; return PCR_ERR_ARG; }
	FLUSH(ctx);                                   // (the launcher thread records the scan events)
	ctx->prof = (on != 0);
	ctx->prof_stride = (on > 1) ? (uint32_t)on : 1u; ctx->prof_pass = 0;
	return PCR_OK;
}

int pcr_profile_read(pcr_ctx *ctx, double *scan_ms, uint64_t *scan_launches, int reset)
{
	if(!ctx){ g_err = "null ctx"; return PCR_ERR_ARG; }
	FLUSH(ctx);
	HIP_TRY(hipStreamSynchronize(ctx->stream));
	for(auto &pr : ctx->prof_events){
		float ms = 0.0f;
		HIP_TRY(hipEventElapsedTime(&ms, pr.first, pr.second));
		ctx->prof_ms += ms; ctx->prof_launches += 1;
	}
	ctx->prof_events.clear();
	if(scan_ms) *scan_ms = ctx->prof_ms;
	if(scan_launches) *scan_launches = ctx->prof_launches;
	if(reset){ ctx->prof_ms = 0.0; ctx->prof_launches = 0; }
	return PCR_OK;
}

int pcr_profile_read_kernel(pcr_ctx *ctx, int kernel, double *ms, uint64_t *launches, int reset)
{
	if(!ctx || kernel < 0 || kernel >= PCR_PROF_KERNELS){ g_err = "pcr_profile_read_kernel: bad argument"; return PCR_ERR_ARG; }
	if(kernel == PCR_PROF_SCAN) return pcr_profile_read(ctx, ms, launches, reset);
	FLUSH(ctx);
	HIP_TRY(hipStreamSynchronize(ctx->stream));
	for(auto &pr : ctx->prof_events_k[kernel]){
		float t = 0.0f;
		HIP_TRY(hipEventElapsedTime(&t, pr.first, pr.second));
		ctx->prof_ms_k[kernel] += t; ctx->prof_launches_k[kernel] += 1;
	}
	ctx->prof_events_k[kernel].clear();
	if(ms) *ms = ctx->prof_ms_k[kernel];
	if(launches) *launches = ctx->prof_launches_k[kernel];
	if(reset){ ctx->prof_ms_k[kernel] = 0.0; ctx->prof_launches_k[kernel] = 0; }
	return PCR_OK;
}

// ------------------------------------------------------------------ host-only helpers
static pcrhost::PackFilter make_filter(const pcr_params *params)
{
	pcrhost::PackFilter f;
	f.max_degen = params ? params->pack_max_degen : 256;
	f.set_gc(params ? params->pack_min_gc : 0.0f, params ? params->pack_max_gc : 1.0f);
	return f;
}

int64_t pcr_host_irregular_words(const uint8_t *packed4, uint64_t len, const pcr_params *params,
	uint32_t min_oligo_length, pcr_entry *out, uint64_t cap)
{
	if(len && !packed4){ g_err = "pcr_host_irregular_words: bad argument"; return PCR_ERR_ARG; }
	std::vector<uint8_t> buf(packed4, packed4 + (len + 1)/2);
	if((len & 1) && !buf.empty()) buf.back() &= 0xF0;
	const pcrhost::PackFilter f = make_filter(params);
	std::vector<pcrhost::IrrEntry> v;
	pcrhost::PackedSeq q; q.buf = buf.data(); q.len = len;
	if(!pcrhost::irregular_words(q, f, v)){ g_err = "irregular word overflow"; return PCR_ERR_CAPACITY; }
	uint64_t n = 0;
	for(const pcrhost::IrrEntry &e : v){
		if(e.cws < min_oligo_length) continue;
		if(n < cap && out){
			pcrhost::word_of_planes(e.w, out[n].word.w);
			out[n].loc = e.loc; out[n].index = 0; out[n].strand = e.strand; out[n].pad = e.ord;
		}
		++n;
	}
	return (int64_t)n;
}

int pcr_host_window_valid(const uint8_t *packed4, uint64_t len, const pcr_params *params, uint8_t *valid_out)
{
	if(len && (!packed4 || !valid_out)){ g_err = "pcr_host_window_valid: bad argument"; return PCR_ERR_ARG; }
	const pcrhost::PackFilter f = make_filter(params);
	pcrhost::PackedSeq q; q.buf = packed4; q.len = len;
	for(uint64_t p = 0;p < len;++p){
		bool ok = (p + 32 <= len);
		unsigned n2 = 0, n3 = 0, n4 = 0, ngc = 0;
		for(int k = 0;ok && k < 32;++k){
			const unsigned v = q.at(p + k);
			if(v == 0){ ok = false; break; }
			const int d = __builtin_popcount(v);
			n2 += (d == 2); n3 += (d == 3); n4 += (d == 4);
			ngc += ((v & 6) != 0);
		}
		if(ok && !((f.gc_ok >> ngc) & 1)) ok = false;
		if(ok && pcrhost::degeneracy_exceeds(n2, n3, n4, f.max_degen)) ok = false;
		valid_out[p] = ok ? 1 : 0;
	}
	return PCR_OK;
}

int64_t pcr_host_candidates(const pcr_pair *pairs, uint32_t n_pairs, int optimize_5, int optimize_3,
	float threshold, pcr_word128 *words_out, uint32_t *floors_out, uint64_t cap)
{
	std::vector<pcrhost::Candidate> cand;
	pcrhost::build_candidates((const uint64_t *)pairs, n_pairs, optimize_5 != 0, optimize_3 != 0, threshold, cand);
	for(size_t i = 0;i < cand.size() && i < cap;++i){
		if(words_out) pcrhost::word_of_planes(cand[i].fwd, words_out[i].w);
		if(floors_out) floors_out[i] = cand[i].floor_;
	}
	return (int64_t)cand.size();
}

int64_t pcr_host_orientation_seeds(const pcr_word128 *oligo, uint32_t floor, uint32_t *codes, uint8_t *q, uint8_t *off, uint64_t cap)
{
	if(!oligo){ g_err = "null oligo"; return PCR_ERR_ARG; }
	std::vector<pcrhost::Seed> seeds;
	if(!pcrhost::orientation_seeds(pcrhost::planes_of_word(oligo->w), floor, 0, seeds)) return -1;
	for(size_t i = 0;i < seeds.size() && i < cap;++i){
		if(codes) codes[i] = seeds[i].code;
		if(q) q[i] = seeds[i].q;
		if(off) off[i] = seeds[i].off;
	}
	return (int64_t)seeds.size();
}

int64_t pcr_host_orientation_fold_seeds(const pcr_word128 *oligo, uint32_t floor, uint32_t *codes, uint8_t *off, uint8_t *lo, uint8_t *hi, uint64_t cap)
{
	if(!oligo){ g_err = "null oligo"; return PCR_ERR_ARG; }
	std::vector<pcrhost::FoldSeed> seeds; std::vector<pcrhost::Seed> tmp;
	if(!pcrhost::orientation_fold_seeds(pcrhost::planes_of_word(oligo->w), floor, seeds, tmp)) return -1;
	for(size_t i = 0;i < seeds.size() && i < cap;++i){
		if(codes) codes[i] = seeds[i].code;
		if(off) off[i] = seeds[i].off;
		if(lo) lo[i] = seeds[i].lo;
		if(hi) hi[i] = seeds[i].hi;
	}
	return (int64_t)seeds.size();
}

int64_t pcr_host_move_trials(const pcr_word128 *oligo, int move, double max_degen, int primer_min, int primer_max,
	pcr_word128 *trials_out, uint64_t cap)
{
	if(!oligo){ g_err = "null oligo"; return PCR_ERR_ARG; }
	std::vector<Planes> t;
	if(!pcrhost::move_trials(pcrhost::planes_of_word(oligo->w), move, max_degen, primer_min, primer_max, t)){
		g_err = "pcr_host_move_trials: unknown move"; return PCR_ERR_ARG;
	}
	for(size_t i = 0;i < t.size() && i < cap;++i) pcrhost::word_of_planes(t[i], trials_out[i].w);
	return (int64_t)t.size();
}

} // extern "C"

#include "pcr_exchange.inc"
#include "pcr_shard.inc"
#include "pcr_trial_ranks.inc"
#include "pcr_entry_sw_thermo.inc"
#include "pcr_multiplex_screen.inc"
#include "pcr_pool.inc"
#include "pcr_site_tm.inc"
#include "pcr_site_variants.inc"
#include "pcr_site_repair.inc"
#include "pcr_pool_dimers.inc"
#include "pcr_pool_dimers_end3.inc"
#include "pcr_products_tm.inc"
#include "pcr_products_end3.inc"
#include "pcr_anneal_profile.inc"
#include "pcr_pool_conflicts.inc"
#include "pcr_pool_conflicts_ext.inc"
#include "pcr_probe_hits.inc"
#include "pcr_pool_amplicons.inc"
#include "pcr_probe_candidates.inc"
#include "pcr_writers.inc"
