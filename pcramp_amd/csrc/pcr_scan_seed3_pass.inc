// The body of k_seed3 and of each row of k_seed3_pair: one pass of the third form as the workgroups of one launch row (blockIdx.x of
// gridDim.x) run it.  Included as TEXT where T3, Q, IA, cand_fwd, cand_floor, sink, Z and W (the row's slices) are in scope, not called:
// as an always-inlined function of these arguments the same statements took k_seed3 from 63 VGPRs and no scratch to 64 and a spilled
// register (profiles/pair_launch.md), and the kernel may use 64 (amdgpu_waves_per_eu(8, 8)).
	extern __shared__ uint4 s3_dyn[];                          // masks [n_or] | the workgroup's slice of chunk_prefix and of the seeds [slice_cap each] | floors [n_or, padded to 16] | the slice of the spans
	uint4 *const masks = s3_dyn;
	uint32_t *const prefix = (uint32_t *)(masks + T3.n_or);
	uint32_t *const seeds = prefix + T3.slice_cap;
	uint8_t *const floors = (uint8_t *)(seeds + T3.slice_cap);
	uint8_t *const spans = floors + ((T3.n_or + 15u) & ~15u);
	// (the wave's number is uniform: held in a scalar register it is not a vector register kept across the chunk loop for the irregular words behind it)
	const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63u;
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
