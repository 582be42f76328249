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
	extern __shared__ uint4 s3_dyn[];                          // masks [n_or] | the workgroup's slice of chunk_prefix and of the seeds [slice_cap each] | floors [n_or, padded to 16] | the slice of the spans
	uint4 *const masks = s3_dyn;
	uint32_t *const prefix = (uint32_t *)(masks + T3.n_or);
	uint32_t *const seeds = prefix + T3.slice_cap;
	uint8_t *const floors = (uint8_t *)(seeds + T3.slice_cap);
	uint8_t *const spans = floors + ((T3.n_or + 15u) & ~15u);
	const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
	// the lean fused pass has no staging launch: what k_seed2 clears in its prologue is cleared here
	for(uint32_t i = blockIdx.x*S3_THREADS + threadIdx.x;i < Z.n0;i += gridDim.x*S3_THREADS) Z.z0[i] = make_uint4(0, 0, 0, 0);
	for(uint32_t i = blockIdx.x*S3_THREADS + threadIdx.x;i < Z.n1;i += gridDim.x*S3_THREADS) Z.z1[i] = make_uint4(0, 0, 0, 0);
	if(Z.ctrl && blockIdx.x == 0 && threadIdx.x == 0){ Z.ctrl[1] = 0; Z.ctrl[3] = 0; }
	for(uint32_t i = threadIdx.x;i < T3.n_or;i += S3_THREADS){ masks[i] = T3.masks[i]; floors[i] = T3.floors[i]; }
	constexpr uint32_t S3_WAVES = S3_THREADS/64;
	if(blockIdx.x < T3.n_irr_wg){                                                  // (uniform per workgroup; no barrier behind this point for it)
		if(IA.ix_first) s3_irregular(T3, Q, IA, cand_fwd, cand_floor, sink, blockIdx.x*S3_WAVES + wave, T3.n_irr_wg*S3_WAVES, lane);
		return;
	}
	const uint32_t wg = blockIdx.x - T3.n_irr_wg, n_wg = gridDim.x - T3.n_irr_wg;     // among the workgroups that read the chunks
	const uint32_t s_lo = W.start[wg];
	const uint32_t n_slice = min(min(W.start[wg + 1] + 2u, T3.n_seeds + 1u) - s_lo, T3.slice_cap);   // list entries s_lo ... start[w + 1] + 1
	for(uint32_t i = threadIdx.x;i < n_slice;i += S3_THREADS){ prefix[i] = T3.chunk_prefix[s_lo + i]; const bool in = s_lo + i < T3.n_seeds; seeds[i] = in ? T3.seeds[s_lo + i] : 0u; spans[i] = in ? T3.spans[s_lo + i] : (uint8_t)0; }
	__syncthreads();
	const uint32_t gw = wg*S3_WAVES + wave, n_gw = n_wg*S3_WAVES;
	const uint32_t q_lo = wg*T3.per_wg, q_hi = min(q_lo + T3.per_wg, T3.n_chunks);
	for(uint32_t q0 = q_lo + wave;q0 < q_hi;q0 += S3_WAVES*S3_BATCH){
		// ---- lane b < S3_BATCH: chunk q0 + b * S3_WAVES -> its seed (the last s with prefix[s] <= q), the seed's run
		uint32_t c_first = 0, c_cnt = 0, c_sd = 0;
		{
			const uint32_t q = q0 + lane*S3_WAVES;
			if(lane < S3_BATCH && q < q_hi){
				uint32_t lo = 0, hi = n_slice - 1u;                                // prefix[lo] <= q < prefix[hi]
				while(hi - lo > 1u){ const uint32_t mid = (lo + hi) >> 1; if(prefix[mid] <= q) lo = mid; else hi = mid; }
				c_sd = seeds[lo];
				const uint32_t key = (c_sd >> 14) << 2, sp = spans[lo];               // sub-runs key + lo .. key + hi
				const uint32_t f = T3.pix_first[key + (sp & 3u)], e = T3.pix_last[key + (sp >> 2)], j0 = (q - prefix[lo])*64u;
				c_first = f + j0; c_cnt = (e - f) - j0;                           // entries of the run from this chunk on (> 0)
			}
		}
		// ---- the chunks' entries (position + context), a coalesced 16-byte read per lane, all of the batch back to back
		uint4 en[S3_BATCH];
#pragma unroll
		for(int b = 0;b < (int)S3_BATCH;++b){
			const uint32_t first = s2_rl(c_first, b), cnt = s2_rl(c_cnt, b);
			en[b] = make_uint4(0xFFFFFFFFu, 0, 0, 0);
			if(lane < cnt) en[b] = T3.pix_ent[first + lane];
		}
		// ---- the exact count of every entry's window, out of the entry; then, for the few that reach their floor, the checks the tile forms
		// make per tile or per window -- in three sweeps over the batch, so that a wave pays their two memory round trips once per turn,
		// not once per chunk that holds a survivor
		uint32_t cnt_b[S3_BATCH], g[S3_BATCH]; bool pass_b[S3_BATCH];
#pragma unroll
		for(int b = 0;b < (int)S3_BATCH;++b){
			const uint32_t sdv = s2_rl(c_sd, b);
			const uint32_t off = (sdv >> 9) & 31u, local = sdv & 0x1FFu, code = sdv >> 14;
			g[b] = en[b].x;
			// the 2-bit codes of bases p - 24 ... p + 39 as four words (p - 24 itself and p + 32 ... are never asked for): left << 2 | key << 48 | right << 66
			const uint32_t r_lo = funnel(en[b].z, en[b].w, 14);
			const uint4 cx = make_uint4(en[b].y << 2, (funnel(en[b].y, en[b].z, 30) & 0xFFFFu) | (code << 16), (code >> 16) | (r_lo << 2), en[b].w >> 12);
			// the window inside the context: 24 - offset bases in
			const uint32_t in = 24u - off, sh = 2u*(in & 15u);
			const uint32_t a0 = (in < 16u) ? funnel(cx.x, cx.y, sh) : funnel(cx.y, cx.z, sh);
			const uint32_t a1 = (in < 16u) ? funnel(cx.y, cx.z, sh) : funnel(cx.z, cx.w, sh);
			cnt_b[b] = (uint32_t)__popc(s2_mux(a0, a1, masks[local]));
			pass_b[b] = g[b] != 0xFFFFFFFFu && cnt_b[b] >= floors[local] && g[b] >= off;   // (a window that would start before the first base: none)
		}
		uint32_t vw[S3_BATCH], info[S3_BATCH], bl[S3_BATCH];
#pragma unroll
		for(int b = 0;b < (int)S3_BATCH;++b){
			vw[b] = 0; info[b] = 0; bl[b] = 0;
			if(pass_b[b]){
				const uint32_t ws = g[b] - ((s2_rl(c_sd, b) >> 9) & 31u);              // window start (global base position)
				vw[b] = Q.valid[ws >> 5]; info[b] = Q.blk_info[ws >> 5]; bl[b] = Q.blk_local[ws >> 5];
			}
		}
#pragma unroll
		for(int b = 0;b < (int)S3_BATCH;++b){
			if(!pass_b[b]) continue;
			const uint32_t sdv = s2_rl(c_sd, b);
			const uint32_t ws = g[b] - ((sdv >> 9) & 31u), seq = info[b] & BLK_SEQ_MASK;
			// inside its sequence, no EOS, degeneracy (k_valid); not in a tile with IUPAC codes (the bit-sliced scan's); an active sequence
			if(!((vw[b] >> (ws & 31u)) & 1u) || (info[b] & (BLK_DEGEN | BLK_INACTIVE))) continue;
			const uint32_t p_local = bl[b]*32u + (ws & 31u);
			const uint32_t orient = T3.or_base + (sdv & 0x1FFu), c = orient >> 1;
			if(orient & 1u) record_hit(sink, seq, c, make_key(seq, (int32_t)p_local + 31, 2, 0, 0), cnt_b[b]);   // sequence.cpp:190
			else record_hit(sink, seq, c, make_key(seq, (int32_t)p_local, 1, 0, 0), cnt_b[b]);                    // sequence.cpp:184
		}
	}
	// ---- the irregular words: by workgroups of their own when the launch has them (the chunk waves' chain and this one then run
	// side by side instead of one after the other), else by the chunk waves afterwards
	if(IA.ix_first && T3.n_irr_wg == 0) s3_irregular(T3, Q, IA, cand_fwd, cand_floor, sink, gw, n_gw, lane);
}
