// C-ABI entry points of the Smith-Waterman family and the thermodynamics (included at the end of pcr_device.hip).
// ------------------------------------------------------------------ Smith-Waterman entry points
namespace {

// SeqOverlap::pack_query_slots (seq_overlap.h:828-857): size() codes starting at start()
int word_codes(const Planes &w, uint8_t *codes)
{
	const int len = pcrhost::planes_size(w), start = pcrhost::planes_start(w);
	for(int k = 0;k < 32;++k) codes[k] = (k < len && start + k < 32) ? (uint8_t)pcrhost::planes_nibble(w, start + k) : 0;
	return len;
}

// queries of pair p: 4p + {0: F, 1: (F), 2: R, 3: (R)} and the per-pair constants of background_match.cpp:20-42
void pair_queries(const pcr_pair *pairs, uint32_t n_pairs, std::vector<uint8_t> &q, std::vector<uint8_t> &ql, std::vector<BgPairDev> &bp)
{
	q.assign((size_t)n_pairs*4*32, 0); ql.assign((size_t)n_pairs*4, 0); bp.assign(n_pairs, BgPairDev());
	for(uint32_t p = 0;p < n_pairs;++p){
		const Planes F = pcrhost::planes_of_word(pairs[p].f.w), R = pcrhost::planes_of_word(pairs[p].r.w);
		const Planes o[4] = {F, pcrhost::planes_revcomp(F), R, pcrhost::planes_revcomp(R)};
		uint8_t last[4][2];
		for(int l = 0;l < 4;++l){
			ql[(size_t)p*4 + l] = (uint8_t)word_codes(o[l], &q[((size_t)p*4 + l)*32]);
			const int stop = pcrhost::planes_stop(o[l]);                          // Word::get_last_two, word.h:299
			last[l][0] = (stop >= 1) ? (uint8_t)pcrhost::planes_nibble(o[l], stop - 1) : 0;
			last[l][1] = (stop >= 0) ? (uint8_t)pcrhost::planes_nibble(o[l], stop) : 0;
		}
		BgPairDev b;
		float f_norm = 2.0f*(unsigned)pcrhost::planes_size(F), r_norm = 2.0f*(unsigned)pcrhost::planes_size(R);   // PERFECT_MATCH_SCORE, assay.h:15
		if(f_norm > 0.0f) f_norm = 1.0f/f_norm;
		if(r_norm > 0.0f) r_norm = 1.0f/r_norm;
		b.f_norm = f_norm; b.r_norm = r_norm;
		b.fp1 = last[0][0]; b.fp2 = last[0][1]; b.fm1 = last[1][0]; b.fm2 = last[1][1];
		b.rp1 = last[2][0]; b.rp2 = last[2][1]; b.rm1 = last[3][0]; b.rm2 = last[3][1];
		bp[p] = b;
	}
}

int upload_pair_queries(pcr_ctx *ctx, const pcr_pair *pairs, uint32_t n_pairs)
{
	std::vector<uint8_t> q, ql; std::vector<BgPairDev> bp;
	pair_queries(pairs, n_pairs, q, ql, bp);
	int rc;
	if((rc = ctx->sw_q.ensure(q.size())) != PCR_OK) return rc;
	if((rc = ctx->sw_qlen.ensure(ql.size())) != PCR_OK) return rc;
	if((rc = ctx->bg_pairs.ensure(bp.size())) != PCR_OK) return rc;
	HIP_TRY(hipMemcpyAsync(ctx->sw_q.p, q.data(), q.size(), hipMemcpyHostToDevice, ctx->stream));
	HIP_TRY(hipMemcpyAsync(ctx->sw_qlen.p, ql.data(), ql.size(), hipMemcpyHostToDevice, ctx->stream));
	HIP_TRY(hipMemcpyAsync(ctx->bg_pairs.p, bp.data(), bp.size()*sizeof(BgPairDev), hipMemcpyHostToDevice, ctx->stream));
	HIP_TRY(hipStreamSynchronize(ctx->stream));
	return PCR_OK;
}

int launch_sw(pcr_ctx *ctx, uint64_t n_jobs, const uint8_t *d_tcodes)
{
	if(n_jobs == 0) return PCR_OK;
	if(n_jobs >= (uint64_t(1) << 31)){ g_err = "too many alignment jobs in one call"; return PCR_ERR_CAPACITY; }
	int rc;
	if((rc = ctx->sw_out.ensure(n_jobs)) != PCR_OK) return rc;
	const unsigned jobs_per_block = SW_THREADS/32;
	ProfScope prof(ctx, PCR_PROF_SW);
	// (both callers -- the background and the multiplex screen -- read the score and the last two aligned template bases only: score-only form)
	hipLaunchKernelGGL(k_sw<false>, dim3((unsigned)((n_jobs + jobs_per_block - 1)/jobs_per_block)), dim3(SW_THREADS), 0, ctx->stream,
		ctx->sw_jobs.p, (uint32_t)n_jobs, ctx->sw_q.p, ctx->sw_qlen.p, d_tcodes, ctx->sw_out.p);
	HIP_TRY(hipGetLastError());
	return PCR_OK;
}

// The candidate amplicons of k_pair_emit in the reference's order (see k_amp_keys): radix sort of the record indices by
// (orientation, sequence, plus site, minus site), then a stable sort by pair, then one gather; *pair_start_out[p] = index of pair p's first record.
int order_amplicons(pcr_ctx *ctx, SeqSet &S, uint32_t n_amp, uint32_t n_pairs, const AmpRec **recs_out, const uint32_t **pair_start_out)
{
	int rc;
	if((rc = ctx->amp_recs2.ensure(n_amp)) != PCR_OK) return rc;
	if((rc = ctx->amp_keys.ensure(2*(size_t)n_amp)) != PCR_OK) return rc;
	if((rc = ctx->amp_pkeys.ensure(4*(size_t)n_amp)) != PCR_OK) return rc;         // pair keys in / out | record indices in / out
	if((rc = ctx->amp_pair_start.ensure(n_pairs)) != PCR_OK) return rc;
	const unsigned grid = (n_amp + 255)/256;
	uint64_t *k0 = ctx->amp_keys.p, *k1 = ctx->amp_keys.p + n_amp;
	uint32_t *p0 = ctx->amp_pkeys.p, *p1 = p0 + n_amp, *i0 = p0 + 2*(size_t)n_amp, *i1 = p0 + 3*(size_t)n_amp;
	unsigned pair_bits = 1; while(pair_bits < 32 && (1ull << pair_bits) < n_pairs) ++pair_bits;
	size_t tmp1 = 0, tmp2 = 0;
	HIP_TRY(rocprim::radix_sort_pairs(nullptr, tmp1, k0, k1, i0, i1, n_amp, 0, 59, ctx->stream));
	HIP_TRY(rocprim::radix_sort_pairs(nullptr, tmp2, p0, p1, i1, i0, n_amp, 0, pair_bits, ctx->stream));
	if((rc = ctx->sort_tmp.ensure(std::max(tmp1, tmp2) + 16)) != PCR_OK) return rc;
	hipLaunchKernelGGL(k_amp_keys, dim3(grid), dim3(256), 0, ctx->stream, ctx->amp_recs.p, n_amp, S.db_cap, k0, i0);
	HIP_TRY(hipGetLastError());
	HIP_TRY(rocprim::radix_sort_pairs(ctx->sort_tmp.p, tmp1, k0, k1, i0, i1, n_amp, 0, 59, ctx->stream));
	hipLaunchKernelGGL(k_amp_pair_keys, dim3(grid), dim3(256), 0, ctx->stream, ctx->amp_recs.p, i1, n_amp, p0);
	HIP_TRY(hipGetLastError());
	HIP_TRY(rocprim::radix_sort_pairs(ctx->sort_tmp.p, tmp2, p0, p1, i1, i0, n_amp, 0, pair_bits, ctx->stream));   // (stable)
	hipLaunchKernelGGL(k_amp_gather, dim3(grid), dim3(256), 0, ctx->stream, ctx->amp_recs.p, i0, n_amp, ctx->amp_recs2.p);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipMemsetAsync(ctx->amp_pair_start.p, 0, n_pairs*sizeof(uint32_t), ctx->stream));
	hipLaunchKernelGGL(k_amp_pair_start, dim3(grid), dim3(256), 0, ctx->stream, ctx->amp_recs2.p, n_amp, ctx->amp_pair_start.p);
	HIP_TRY(hipGetLastError());
	*recs_out = ctx->amp_recs2.p; *pair_start_out = ctx->amp_pair_start.p;
	return PCR_OK;
}

} // namespace

extern "C" {

int pcr_sw_align_words(pcr_ctx *ctx, const pcr_word128 *queries, const pcr_word128 *templates, uint32_t n, pcr_sw_result *out)
{
	if(!ctx || (n && (!queries || !templates || !out))){ g_err = "pcr_sw_align_words: bad argument"; return PCR_ERR_ARG; }
	if(n == 0) return PCR_OK;
	FLUSH(ctx);
	HIP_TRY(hipSetDevice(ctx->device));
	static_assert(sizeof(SwOut) == sizeof(pcr_sw_result), "result layout");
	// The words go to the device as they are (the kernel reads the code strings out of them) through two pinned,
	// host-mapped chunk buffers: while the GPU aligns chunk k the host copies chunk k + 1 in and chunk k - 1 out, so
	// the call lasts about as long as the slower of the two (host copies ~ PCIe + kernel), not their sum.
	const uint32_t CH = 1u << 16;                                                  // lanes per chunk: 2 MB of words, 1 MB of results
	{ const int rc = ctx->sw_pin.ensure(2*(size_t)CH*(2*sizeof(pcr_word128) + sizeof(SwOut))); if(rc != PCR_OK) return rc; }
	for(int k = 0;k < 2;++k){ if(!ctx->sw_done[k]) HIP_TRY(ctx->sw_done[k].create(hipEventDisableTiming)); }
	const size_t slot_bytes = (size_t)CH*(2*sizeof(pcr_word128) + sizeof(SwOut));
	const uint32_t n_chunks = (n + CH - 1)/CH;
	auto host_q = [&](uint32_t k){ return (pcr_word128 *)(ctx->sw_pin.host + (k & 1u)*slot_bytes); };
	auto copy_out = [&](uint32_t c) -> int {
		HIP_TRY(hipEventSynchronize(ctx->sw_done[c & 1u]));
		const uint32_t lo = c*CH, cnt = std::min(CH, n - lo);
		memcpy(out + lo, (const uint8_t *)host_q(c) + (size_t)CH*2*sizeof(pcr_word128), (size_t)cnt*sizeof(SwOut));
		return PCR_OK;
	};
	for(uint32_t c = 0;c < n_chunks;++c){
		int rc;
		if(c >= 2 && (rc = copy_out(c - 2)) != PCR_OK) return rc;                   // its slot is reused now
		const uint32_t lo = c*CH, cnt = std::min(CH, n - lo);
		pcr_word128 *hq = host_q(c), *ht = hq + CH;
		memcpy(hq, queries + lo, (size_t)cnt*sizeof(pcr_word128));
		memcpy(ht, templates + lo, (size_t)cnt*sizeof(pcr_word128));
		const uint8_t *dev = ctx->sw_pin.dev + (c & 1u)*slot_bytes;
		const unsigned jobs_per_block = SW_THREADS/32;
		{
			ProfScope prof(ctx, PCR_PROF_SW);
			hipLaunchKernelGGL(k_sw_words, dim3((cnt + jobs_per_block - 1)/jobs_per_block), dim3(SW_THREADS), 0, ctx->stream,
				(const pcr_word128 *)dev, (const pcr_word128 *)dev + CH, cnt, (SwOut *)(dev + (size_t)CH*2*sizeof(pcr_word128)));
			HIP_TRY(hipGetLastError());
		}
		HIP_TRY(hipEventRecord(ctx->sw_done[c & 1u], ctx->stream));
	}
	for(uint32_t c = (n_chunks >= 2) ? n_chunks - 2 : 0;c < n_chunks;++c){ const int rc = copy_out(c); if(rc != PCR_OK) return rc; }
	return PCR_OK;
}

static int background_match_ordered(pcr_ctx *ctx, SeqSet &S, const pcr_pair *pairs, uint32_t n_pairs, const pcr_background_args *args, uint64_t *bits);

int pcr_background_match(pcr_ctx *ctx, pcr_set which, const pcr_pair *pairs, uint32_t n_pairs, const pcr_background_args *args,
	uint64_t *bits)
{
	if(!set_ok(which)){ g_err = "pcr_background_match: unknown sequence set"; return PCR_ERR_ARG; }
	if(!ctx || !args || (n_pairs && (!pairs || !bits))){ g_err = "pcr_background_match: bad argument"; return PCR_ERR_ARG; }
	DRAIN(ctx);
	HIP_TRY(hipSetDevice(ctx->device));
	SeqSet &S = ctx->sets[which];
	if(!S.have_db){ g_err = "pcr_background_match: no word DB (call pcr_select_words first)"; return PCR_ERR_STATE; }
	// k_bg_emit keeps the batch's oligo geometry in LDS, 8 bytes per pair beside its own arrays (a batch of more than 32 * BGE_MW oligos
	// runs the <0> form): the batch must fit what a workgroup of this device may declare.  Asked of the runtime once per handle.
	if(!ctx->bg_max_pairs){
		int lds_max = 0;
		hipFuncAttributes fa;
		HIP_TRY(hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, ctx->device));
		HIP_TRY(hipFuncGetAttributes(&fa, (const void *)k_bg_emit<0>));
		if(lds_max <= 0 || (size_t)lds_max <= fa.sharedSizeBytes){ g_err = "pcr_background_match: the device reports too little LDS per workgroup"; return PCR_ERR_DEVICE; }
		HIP_TRY(hipFuncSetAttribute((const void *)k_bg_emit<0>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)((size_t)lds_max - fa.sharedSizeBytes)));
		ctx->bg_max_pairs = (uint32_t)(((size_t)lds_max - fa.sharedSizeBytes)/(2*sizeof(uint32_t)));
	}
	if(n_pairs > ctx->bg_max_pairs){
		g_err = "pcr_background_match: too many pairs in one call: at most " + std::to_string(ctx->bg_max_pairs) + " pairs (the LDS of a workgroup holds the batch's oligo geometry)";
		return PCR_ERR_CAPACITY;
	}
	{ const int erc = ensure_touched(ctx, S); if(erc != PCR_OK) return erc; }
	const uint64_t words = (S.n + 63)/64;
	const size_t total = (size_t)n_pairs*words;
	if(total) memset(bits, 0, total*sizeof(uint64_t));
	if(S.n_entries == 0 || n_pairs == 0) return PCR_OK;
	int rc;
	// ---- the default path: no host round trip between the kernels, no sort.  The candidate amplicons are emitted in whatever
	// order the waves get there; the reference's `(i + 1) >= num_seq` rule (background_match.cpp:122) can only drop an amplicon
	// of a pair that has MORE candidate amplicons than there are sequences, so as long as no pair has (k_bg_score looks at the
	// per-pair counts) every amplicon counts and the order is immaterial.  A pair beyond that -- or a caller who wants every
	// amplicon anyway -- and the list's overflow are the two ways out: the latter repeats with a larger list, the former takes
	// the ordered path below (rocprim radix sorts: the one library primitive of the library, on this rare path only).
	for(int attempt = 0;attempt < 6;++attempt){
		const float thr2 = args->collect_threshold*args->collect_threshold;
		std::vector<OligoDev> ol(2*(size_t)n_pairs);
		for(uint32_t i = 0;i < n_pairs;++i){ fill_oligo(ol[2*i], pairs[i].f.w, thr2); fill_oligo(ol[2*i + 1], pairs[i].r.w, thr2); }
		std::vector<uint8_t> q, ql; std::vector<BgPairDev> bp;
		pair_queries(pairs, n_pairs, q, ql, bp);
		const uint32_t mask_words = (2*n_pairs + 31)/32;
		if((rc = ctx->mask.ensure((size_t)S.n_slots*mask_words)) != PCR_OK) return rc;
		if((rc = ctx->status.ensure(1)) != PCR_OK) return rc;
		if((rc = ctx->counters.ensure(4 + (size_t)n_pairs + BGE_SUB + 4)) != PCR_OK) return rc;      // [0] records, [1] flags, [2] overflow | per-pair record counts | sub-list fills
		if((rc = ctx->amp_recs2.ensure(ctx->amp_cap)) != PCR_OK) return rc;                 // the sub-lists (amp_cap / BGE_SUB records each)
		if((rc = ctx->bits_fr.ensure(total + 2)) != PCR_OK) return rc;
		if((rc = ctx->amp_recs.ensure(ctx->amp_cap)) != PCR_OK) return rc;
		if((rc = ctx->sw_out.ensure(4*ctx->amp_cap)) != PCR_OK) return rc;
		Stager st(ctx);
		if((rc = st.begin(ol.size()*sizeof(OligoDev) + q.size() + ql.size() + bp.size()*sizeof(BgPairDev) + 256)) != PCR_OK) return rc;
		const OligoDev *d_ol = st.put(ol.data(), ol.size());
		const uint8_t *d_q = st.put(q.data(), q.size());
		const uint8_t *d_ql = st.put(ql.data(), ql.size());
		const BgPairDev *d_bp = st.put(bp.data(), bp.size());
		if((rc = st.ship(ctx->counters.p, (4 + (size_t)n_pairs + BGE_SUB)*sizeof(uint32_t), ctx->bits_fr.p, total*sizeof(uint64_t), ctx->status.p, sizeof(uint32_t))) != PCR_OK) return rc;   // (the staging launch clears counters, result bits and the status word)
		// the wave stages its sequence in LDS and computes the masks itself when the buckets are small enough (64 slots is the default)
		const int stage = (mask_words <= (uint32_t)BGE_MW) ? ((S.db_cap <= 64u) ? 64 : (S.db_cap <= 128u) ? 128 : 0) : 0;
		const uint32_t per_cu = (stage == 64) ? 7u : (stage == 128) ? 4u : 8u;                 // workgroups resident per CU (LDS)
		const dim3 egrid(std::max(1u, std::min<uint32_t>((S.n_touched + BGE_WAVES - 1)/BGE_WAVES, ctx->n_cu*per_cu))), eblock(64*BGE_WAVES);
		const uint32_t sub_cap = (uint32_t)(ctx->amp_cap/BGE_SUB);
		uint32_t *const d_pair_count = ctx->counters.p + 4, *const d_sub_count = ctx->counters.p + 4 + n_pairs;
		const size_t geom_bytes = 2*(size_t)n_pairs*sizeof(uint32_t);
#define BGE_ARGS S.db.p, S.n_touched, S.db_cap, S.touched.p, S.d_seg_hi, ctx->mask.p, mask_words, d_ol, n_pairs, S.planes.p, S.d_blk_off.p, S.d_len.p, S.d_active.p, S.d_has_eos.p, \
	args->amp_min, args->amp_max, ctx->amp_recs2.p, sub_cap, d_sub_count, ctx->status.p
		if(stage == 64) hipLaunchKernelGGL(k_bg_emit<64>, egrid, eblock, geom_bytes, ctx->stream, BGE_ARGS);
		else if(stage == 128) hipLaunchKernelGGL(k_bg_emit<128>, egrid, eblock, geom_bytes, ctx->stream, BGE_ARGS);
		else{
			hipLaunchKernelGGL(k_match, dim3((S.n_touched + MATCH_WAVES - 1)/MATCH_WAVES), dim3(64*MATCH_WAVES), 0, ctx->stream, S.db.p, S.n_touched, (const uint32_t *)nullptr, S.db_cap,
				S.touched.p, S.d_seg_hi, d_ol, 2*n_pairs, mask_words, ctx->mask.p, ctx->status.p, (const uint32_t *)nullptr, (pcr_ctx::Mail *)nullptr, 0u);
			HIP_TRY(hipGetLastError());
			hipLaunchKernelGGL(k_bg_emit<0>, egrid, eblock, geom_bytes, ctx->stream, BGE_ARGS);
		}
#undef BGE_ARGS
		HIP_TRY(hipGetLastError());
		hipLaunchKernelGGL(k_bg_compact, dim3(8), dim3(1024), 0, ctx->stream, ctx->amp_recs2.p, sub_cap, d_sub_count, ctx->amp_recs.p, ctx->counters.p, d_pair_count, n_pairs);
		HIP_TRY(hipGetLastError());
		{
			ProfScope prof(ctx, PCR_PROF_SW);
			hipLaunchKernelGGL(k_sw_bg, dim3(ctx->n_cu*8), dim3(SW_THREADS), 0, ctx->stream, ctx->amp_recs.p, ctx->counters.p, (uint32_t)ctx->amp_cap, S.db.p, d_q, d_ql, ctx->sw_out.p);
			HIP_TRY(hipGetLastError());
		}
		hipLaunchKernelGGL(k_bg_score, dim3(ctx->n_cu*4), dim3(256), 0, ctx->stream, ctx->amp_recs.p, (uint32_t)ctx->amp_cap, ctx->counters.p, ctx->sw_out.p, d_bp,
			args->background_threshold, args->use_taq_mama, ctx->bits_fr.p, words, (const uint32_t *)nullptr, S.n,
			args->evaluate_all_amplicons ? (const uint32_t *)nullptr : ctx->counters.p + 4, ctx->counters.p + 1);
		HIP_TRY(hipGetLastError());
		const uint8_t *back[3];
		if((rc = return_to_host(ctx, ctx->bits_fr.p, total*sizeof(uint64_t), ctx->counters.p, 4*sizeof(uint32_t), ctx->status.p, sizeof(uint32_t), back)) != PCR_OK) return rc;
		const uint32_t *cnt = (const uint32_t *)back[1];
		const uint32_t n_amp = cnt[3], flags = cnt[1], status = *(const uint32_t *)back[2];
		if(status & 1u){ g_err = "Sequence::has_split: range is out of bounds"; return PCR_ERR_RANGE; }
		const bool repeat = n_amp > ctx->amp_cap || (cnt[2] & 1u);
		if(ctx->debug_log) fprintf(stderr, "[pcramp] background_match: attempt %d, emit<%d>, %u-slot buckets, %u pairs, list of %zu records in sub-lists of %u, %u records emitted, %u kept, overflow %u: %s\n",
			attempt, stage, S.db_cap, n_pairs, ctx->amp_cap, sub_cap, n_amp, cnt[0], (unsigned)(cnt[2] & 1u), repeat ? "repeated" : (flags & 2u) ? "ordered path" : "default path");
		if(repeat){
			if(n_amp > (1u << 29)){ g_err = "pcr_background_match: candidate amplicon list does not fit"; return PCR_ERR_CAPACITY; }
			ctx->amp_cap = std::max<size_t>(2*ctx->amp_cap, 2*(size_t)n_amp);            // (a sub-list may overflow before the sum does: twice the room)
			continue;
		}
		if(flags & 2u) return background_match_ordered(ctx, S, pairs, n_pairs, args, bits);
		memcpy(bits, back[0], total*sizeof(uint64_t));
		return PCR_OK;
	}
	g_err = "pcr_background_match: candidate amplicon list does not fit"; return PCR_ERR_CAPACITY;
}

// The reference-identical path for a batch in which some pair has more candidate amplicons than there are sequences: the records
// are put into the reference's order per pair and the odd-indexed ones beyond the sequence count are dropped.
// PCR::collect_candidates (pcr_assay.cpp:12-69) for a batch of pairs on set S: the candidate amplicons, as records in device memory
// (*n_amp_out of them at ctx->amp_recs, any order).  match_words of every oligo against the DB at collect_threshold^2 (:31-32).
static int candidate_amplicons(pcr_ctx *ctx, SeqSet &S, const pcr_pair *pairs, uint32_t n_pairs, float collect_threshold, int32_t amp_min, int32_t amp_max,
	uint32_t *n_amp_out)
{
	int rc;
	const float thr2 = collect_threshold*collect_threshold;
	std::vector<OligoDev> ol(2*(size_t)n_pairs);
	for(uint32_t i = 0;i < n_pairs;++i){ fill_oligo(ol[2*i], pairs[i].f.w, thr2); fill_oligo(ol[2*i + 1], pairs[i].r.w, thr2); }
	if((rc = ctx->oligos.ensure(ol.size())) != PCR_OK) return rc;
	HIP_TRY(hipMemcpyAsync(ctx->oligos.p, ol.data(), ol.size()*sizeof(OligoDev), hipMemcpyHostToDevice, ctx->stream));
	HIP_TRY(hipStreamSynchronize(ctx->stream));
	const uint32_t mask_words = (2*n_pairs + 31)/32;
	if((rc = ctx->mask.ensure((size_t)S.n_slots*mask_words)) != PCR_OK) return rc;
	if((rc = ctx->status.ensure(1)) != PCR_OK) return rc;
	if((rc = ctx->counters.ensure(4)) != PCR_OK) return rc;
	const unsigned threads = 128;
	const uint32_t n_db = S.n_touched*S.db_cap;
	const unsigned grid = (n_db + threads - 1)/threads;
	hipLaunchKernelGGL(k_match, dim3((S.n_touched + MATCH_WAVES - 1)/MATCH_WAVES), dim3(64*MATCH_WAVES), 0, ctx->stream, S.db.p, S.n_touched, (const uint32_t *)nullptr, S.db_cap,
		S.touched.p, S.d_seg_hi, ctx->oligos.p, 2*n_pairs, mask_words, ctx->mask.p, (uint32_t *)nullptr, (const uint32_t *)nullptr, (pcr_ctx::Mail *)nullptr, 0u);
	HIP_TRY(hipGetLastError());
	uint32_t n_amp = 0, status = 0;
	for(int attempt = 0;;++attempt){
		if((rc = ctx->amp_recs.ensure(ctx->amp_cap)) != PCR_OK) return rc;
		HIP_TRY(hipMemsetAsync(ctx->counters.p, 0, 4*sizeof(uint32_t), ctx->stream));
		HIP_TRY(hipMemsetAsync(ctx->status.p, 0, sizeof(uint32_t), ctx->stream));
		hipLaunchKernelGGL(k_pair_emit, dim3(grid), dim3(threads), 0, ctx->stream, S.db.p, n_db, S.db_cap, S.touched.p, S.d_seg_hi, ctx->mask.p, mask_words,
			ctx->oligos.p, n_pairs, S.planes.p, S.d_blk_off.p, S.d_len.p, S.d_active.p, amp_min, amp_max,
			ctx->amp_recs.p, (uint32_t)ctx->amp_cap, ctx->counters.p, ctx->status.p);
		HIP_TRY(hipGetLastError());
		HIP_TRY(hipMemcpyAsync(&n_amp, ctx->counters.p, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
		HIP_TRY(hipMemcpyAsync(&status, ctx->status.p, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
		HIP_TRY(hipStreamSynchronize(ctx->stream));
		if(ctx->debug_log) fprintf(stderr, "[pcramp] candidate_amplicons: attempt %d, %u pairs, list of %zu records, %u records emitted: %s\n",
			attempt, n_pairs, ctx->amp_cap, n_amp, (n_amp <= ctx->amp_cap) ? "done" : "repeated");
		if(n_amp <= ctx->amp_cap) break;
		if(attempt >= 4 || n_amp > (1u << 29)){ g_err = "candidate amplicon list does not fit"; return PCR_ERR_CAPACITY; }
		ctx->amp_cap = (size_t)n_amp + (n_amp >> 3);
	}
	if(status & 1u){ g_err = "Sequence::has_split: range is out of bounds"; return PCR_ERR_RANGE; }
	*n_amp_out = n_amp;
	return PCR_OK;
}

static int background_match_ordered(pcr_ctx *ctx, SeqSet &S, const pcr_pair *pairs, uint32_t n_pairs, const pcr_background_args *args, uint64_t *bits)
{
	const uint64_t words = (S.n + 63)/64;
	const size_t total = (size_t)n_pairs*words;
	int rc;
	uint32_t n_amp = 0;
	if((rc = candidate_amplicons(ctx, S, pairs, n_pairs, args->collect_threshold, args->amp_min, args->amp_max, &n_amp)) != PCR_OK) return rc;
	if((rc = upload_pair_queries(ctx, pairs, n_pairs)) != PCR_OK) return rc;
	if((rc = ctx->bits_fr.ensure(total)) != PCR_OK) return rc;
	const uint32_t n_db = S.n_touched*S.db_cap;
	if(n_amp == 0) return PCR_OK;
	if((rc = ctx->entry_codes.ensure((size_t)S.n_slots*32)) != PCR_OK) return rc;
	if((rc = ctx->entry_lens.ensure(S.n_slots)) != PCR_OK) return rc;
	if((rc = ctx->sw_jobs.ensure((size_t)n_amp*4)) != PCR_OK) return rc;
	hipLaunchKernelGGL(k_entry_codes, dim3((unsigned)(((size_t)n_db*32 + 255)/256)), dim3(256), 0, ctx->stream, S.db.p, n_db, S.db_cap, S.touched.p, S.d_seg_hi, ctx->entry_codes.p, ctx->entry_lens.p);
	HIP_TRY(hipGetLastError());
	const AmpRec *d_recs = ctx->amp_recs.p;
	const uint32_t *d_pair_start = nullptr;
	if(!args->evaluate_all_amplicons){
		if((rc = order_amplicons(ctx, S, n_amp, n_pairs, &d_recs, &d_pair_start)) != PCR_OK) return rc;
	}
	hipLaunchKernelGGL(k_bg_jobs, dim3((n_amp*4 + 255)/256), dim3(256), 0, ctx->stream, d_recs, n_amp, ctx->entry_lens.p, ctx->sw_jobs.p);
	HIP_TRY(hipGetLastError());
	if((rc = launch_sw(ctx, (uint64_t)n_amp*4, ctx->entry_codes.p)) != PCR_OK) return rc;
	HIP_TRY(hipMemsetAsync(ctx->bits_fr.p, 0, total*sizeof(uint64_t), ctx->stream));
	hipLaunchKernelGGL(k_bg_score, dim3((n_amp + 255)/256), dim3(256), 0, ctx->stream, d_recs, n_amp, (const uint32_t *)nullptr, ctx->sw_out.p, ctx->bg_pairs.p,
		args->background_threshold, args->use_taq_mama, ctx->bits_fr.p, words, d_pair_start, S.n, (const uint32_t *)nullptr, (uint32_t *)nullptr);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipMemcpyAsync(bits, ctx->bits_fr.p, total*sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
	HIP_TRY(hipStreamSynchronize(ctx->stream));
	return PCR_OK;
}

static int multiplex_match_impl(pcr_ctx *ctx, int which, const pcr_pair *pairs, uint32_t n_pairs, float background_threshold,
	int use_taq_mama, uint64_t *bits);

int pcr_multiplex_match(pcr_ctx *ctx, pcr_set which, const pcr_pair *pairs, uint32_t n_pairs, float background_threshold,
	int use_taq_mama, uint64_t *bits)
{
	if(!set_ok(which)){ g_err = "pcr_multiplex_match: unknown sequence set"; return PCR_ERR_ARG; }
	return multiplex_match_impl(ctx, (int)which, pairs, n_pairs, background_threshold, use_taq_mama, bits);
}

static int multiplex_match_impl(pcr_ctx *ctx, int which, const pcr_pair *pairs, uint32_t n_pairs, float background_threshold,
	int use_taq_mama, uint64_t *bits)
{
	if(!ctx || (n_pairs && (!pairs || !bits))){ g_err = "pcr_multiplex_match: bad argument"; return PCR_ERR_ARG; }
	DRAIN(ctx);
	HIP_TRY(hipSetDevice(ctx->device));
	SeqSet &S = ctx->sets[which];
	const uint64_t words = (S.n + 63)/64;
	const size_t total = (size_t)n_pairs*words;
	if(total) memset(bits, 0, total*sizeof(uint64_t));
	if(S.n == 0 || n_pairs == 0) return PCR_OK;
	int rc;
	std::vector<uint64_t> code_off(S.n);
	uint64_t tot = 0;
	for(uint32_t s = 0;s < S.n;++s){
		// SeqOverlap counts columns in SO_Score (int16) with `j <= max_target_len` (seq_overlap.cpp:383,427): at 32767 the reference never returns
		if(S.len[s] > 32766){ g_err = "pcr_multiplex_match: template longer than 32766 bases, the reference's limit (SeqOverlap's int16 column counter cannot pass 32767)"; return PCR_ERR_CAPACITY; }
		code_off[s] = tot; tot += S.len[s];
	}
	if(!S.have_codes){
		if((rc = S.codes.ensure(tot + 64)) != PCR_OK) return rc;
		if((rc = S.d_code_off.ensure(S.n)) != PCR_OK) return rc;
		HIP_TRY(hipMemcpyAsync(S.d_code_off.p, code_off.data(), S.n*sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
		HIP_TRY(hipStreamSynchronize(ctx->stream));
		if((uint64_t)S.n*SEQ_CODE_SLICES >= (uint64_t(1) << 31)){ g_err = "pcr_multiplex_match: too many sequences in the set"; return PCR_ERR_CAPACITY; }
		hipLaunchKernelGGL(k_seq_codes, dim3(S.n*SEQ_CODE_SLICES), dim3(256), 0, ctx->stream, S.nib.p, S.d_blk_off.p, S.d_len.p, S.d_code_off.p, S.n, S.codes.p);
		HIP_TRY(hipGetLastError());
		S.have_codes = true;
	}
	if((rc = upload_pair_queries(ctx, pairs, n_pairs)) != PCR_OK) return rc;
	const uint64_t n_jobs = (uint64_t)n_pairs*S.n*4;
	if((rc = ctx->sw_jobs.ensure(n_jobs)) != PCR_OK) return rc;
	if((rc = ctx->bits_fr.ensure(total)) != PCR_OK) return rc;
	hipLaunchKernelGGL(k_mx_jobs, dim3((unsigned)((n_jobs + 255)/256)), dim3(256), 0, ctx->stream, n_pairs, S.n, S.d_len.p, S.d_code_off.p, ctx->sw_jobs.p);
	HIP_TRY(hipGetLastError());
	if((rc = launch_sw(ctx, n_jobs, S.codes.p)) != PCR_OK) return rc;
	HIP_TRY(hipMemsetAsync(ctx->bits_fr.p, 0, total*sizeof(uint64_t), ctx->stream));
	hipLaunchKernelGGL(k_mx_score, dim3((unsigned)(((uint64_t)n_pairs*S.n + 255)/256)), dim3(256), 0, ctx->stream, n_pairs, S.n, ctx->sw_out.p,
		ctx->bg_pairs.p, background_threshold, use_taq_mama, ctx->bits_fr.p, words);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipMemcpyAsync(bits, ctx->bits_fr.p, total*sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
	HIP_TRY(hipStreamSynchronize(ctx->stream));
	return PCR_OK;
}

} // extern "C"

// ------------------------------------------------------------------ thermodynamics entry points
namespace {

// NucCruc::update_dp_param (nuc_cruc.cpp:191-342): the integer dG table of the alignment DP at
// 37 C for a given salt.  Float arithmetic in the reference's order; log() is the float overload.
void build_dg_table(float na, int *dg /* [49*49] */)
{
	using namespace thermo;
	auto scale = [](float x){ return (int)(x*10000.0f); };                       // NC_SCORE_SCALE, nuc_cruc.h:235
	const float sc = PCR_SALT*logf(na);
	const float loop_sc = sc*PCR_SUPP_SALT[0], bulge_sc = sc*PCR_SUPP_SALT[1];
	const float match_sc = sc*PCR_SUPP_SALT[2], mismatch_sc = sc*PCR_SUPP_SALT[3];
	for(int i = 0;i < 49*49;++i) dg[i] = scale(PCR_NN_H[i] - TARGET_T*(PCR_NN_S[i] + sc));
	for(int i = bA;i <= bI;++i) for(int j = bA;j <= bI;++j){
		const int curr = i*NB + j;
		for(int k = bA;k <= bI;++k){
			const int prev1 = k*NB + bGAP, prev2 = bGAP*NB + k;
			int v;
			if(PCR_WC[curr]){
				if(curr == pAT || curr == pTA) v = scale(PCR_SUPP[4] - TARGET_T*(PCR_SUPP[5] + match_sc));
				else if(curr == pGC || curr == pCG) v = scale(PCR_SUPP[6] - TARGET_T*(PCR_SUPP[7] + match_sc));
				else v = scale(PCR_SUPP[8] - TARGET_T*(PCR_SUPP[9] + match_sc));
			}
			else v = scale(PCR_SUPP[10] - TARGET_T*(PCR_SUPP[11] + mismatch_sc));
			v = std::max(0, v);
			dg[curr*49 + prev1] = dg[prev1*49 + curr] = dg[curr*49 + prev2] = dg[prev2*49 + curr] = v;
		}
		for(int k = bA;k <= bI;++k) for(int l = bA;l <= bI;++l){
			const int prev = k*NB + l;
			if(!PCR_WC[curr] && !PCR_WC[prev]) dg[curr*49 + prev] = std::max(0, scale(PCR_SUPP[0] - TARGET_T*(PCR_SUPP[1] + loop_sc)));
		}
	}
	for(int i = bA;i <= bI;++i) for(int j = bA;j <= bI;++j){
		const int v = std::max(0, scale(PCR_SUPP[2] - TARGET_T*(PCR_SUPP[3] + bulge_sc)));
		dg[(i*NB + bGAP)*49 + (j*NB + bGAP)] = v;
		dg[(bGAP*NB + i)*49 + (bGAP*NB + j)] = v;
	}
}

// The engine's dG table for `salt` in ctx->th_dg, which every launch of the engine's kernels reads.  It depends on the salt only: the
// handle keeps it on the device between calls and rebuilds it when the salt changes.  st: the stream to work on (default: the handle's).
int ensure_dg_table(pcr_ctx *ctx, float salt, hipStream_t st = nullptr)
{
	if(!st) st = ctx->stream;
	const int rc = ctx->th_dg.ensure(49*49);
	if(rc != PCR_OK) return rc;
	if(ctx->th_dg_salt != salt){
		int dg[49*49];
		build_dg_table(salt, dg);
		HIP_TRY(hipMemcpyAsync(ctx->th_dg.p, dg, sizeof(dg), hipMemcpyHostToDevice, st));
		HIP_TRY(hipStreamSynchronize(st));                                          // dg[] is a stack array
		ctx->th_dg_salt = salt;
	}
	return PCR_OK;
}

// PCR::is_valid's verdict on one expansion's results, and NucCruc::delta_G of its perfect-match duplex: what pcr_thermo reports,
// on the host and in the kernels that reduce the verdict on the device (pcr_probe_candidates.inc).  The library is built with
// -ffp-contract=off: the product and the difference round separately on both sides.
__host__ __device__ inline bool thermo_expansion_valid(const thermo::JobOut &o, const pcr_thermo_args &a, int check_homo_dimer)
{
	if(o.tm_pm < a.tm_min || o.tm_pm > a.tm_max) return false;                    // valid_pcr.cpp:19-23
	if(o.tm_hairpin > a.max_hairpin) return false;                                // :27-31
	if(check_homo_dimer && o.tm_dimer > a.max_dimer) return false;                // :34-41
	return true;
}
__host__ __device__ inline float thermo_delta_g(const thermo::JobOut &o)
{
	return o.dH_pm - thermo::TARGET_T*o.dS_pm;                                     // nuc_cruc.h:1375-1378 (float product, float difference)
}

bool job_set(unsigned char *dst, unsigned char &len, const std::vector<uint8_t> &s)
{
	if(s.empty() || s.size() > (size_t)thermo::MAXL) return false;
	for(size_t i = 0;i < s.size();++i){ if(s[i] > 3) return false; dst[i] = s[i]; }
	len = (unsigned char)s.size();
	return true;
}

// One launch of thermo::k_thermo_wave over n jobs: blocks of THERMO_WAVES independent waves, at most one block per CU (a block takes
// most of a CU's LDS), the waves striding over the jobs.  PCRAMP_THERMO_TIMING=1: the waves' cycles by phase, printed per launch.
int launch_thermo(pcr_ctx *ctx, const thermo::Job *d_jobs, size_t n_jobs, size_t n_mirror, float log_na, const thermo::ThermoValid &V, hipStream_t st = nullptr)
{
	if(!st) st = ctx->stream;
	static const bool timing = getenv("PCRAMP_THERMO_TIMING") != nullptr;
	if(!ctx->th_attr_set){
		HIP_TRY(hipFuncSetAttribute((const void *)thermo::k_thermo_wave, hipFuncAttributeMaxDynamicSharedMemorySize, (int)thermo::THERMO_LDS));
		ctx->th_attr_set = true;
	}
	const size_t n = n_jobs + n_mirror;
	const unsigned nb = (unsigned)std::min<size_t>((n + thermo::THERMO_WAVES - 1)/thermo::THERMO_WAVES, (size_t)ctx->n_cu);
	unsigned long long *dbg = nullptr;
	if(timing){
		int rc;
		if((rc = ctx->th_dbg.ensure(4)) != PCR_OK) return rc;
		HIP_TRY(hipMemsetAsync(ctx->th_dbg.p, 0, 4*sizeof(unsigned long long), st));
		dbg = ctx->th_dbg.p;
	}
	hipLaunchKernelGGL(thermo::k_thermo_wave, dim3(std::max(nb, 1u)), dim3(thermo::THERMO_THREADS), thermo::THERMO_LDS, st, d_jobs, (unsigned)n_jobs, (unsigned)n_mirror,
		ctx->th_dg.p, log_na, ctx->th_out.p, V, dbg);
	HIP_TRY(hipGetLastError());
	if(timing){
		unsigned long long c[4];
		HIP_TRY(hipMemcpyAsync(c, dbg, sizeof(c), hipMemcpyDeviceToHost, st));
		HIP_TRY(hipStreamSynchronize(st));
		const double tot = (double)(c[0] + c[1] + c[2] + c[3]) + 1.0;
		fprintf(stderr, "thermo launch: %zu jobs, %u blocks; wave cycles: fill %.1f%% collect %.1f%% enumerate %.1f%% other %.1f%% (%.0f cycles per job)\n",
			n, nb, 100.0*c[0]/tot, 100.0*c[1]/tot, 100.0*c[2]/tot, 100.0*c[3]/tot, tot/(double)n);
	}
	return PCR_OK;
}

int run_thermo_jobs(pcr_ctx *ctx, const std::vector<thermo::Job> &jobs_in, float salt, std::vector<thermo::JobOut> &out)
{
	out.resize(jobs_in.size());
	if(jobs_in.empty()) return PCR_OK;
	if(!(salt >= 1.0e-6f && salt <= 1.0f)){ g_err = "thermo: salt outside [1e-6, 1] (NucCruc::salt, nuc_cruc.h:780-788)"; return PCR_ERR_ARG; }
	const size_t n_in = jobs_in.size();
	// One job per wave (thermo::k_thermo_wave, grid-stride over the jobs).  A launch lasts as long as its longest job, and
	// that is an oligo job with the homodimer test (hairpin enumeration, then homodimer enumeration): its homodimer half
	// becomes a job of its own (mode 2) on another wave.  When EVERY job is such an oligo job (pcr_thermo with the
	// homodimer check) the kernel mirrors the records itself; otherwise the halves are appended here.
	bool mirror = true;
	for(size_t i = 0;i < n_in && mirror;++i) mirror = (jobs_in[i].mode & ~thermo::JOB_PACKED) == 0 && jobs_in[i].check_homo;
	std::vector<thermo::Job> split;
	std::vector<uint32_t> homo_of;
	if(!mirror){
		split = jobs_in;
		homo_of.assign(n_in, UINT32_MAX);
		for(size_t i = 0;i < n_in;++i){
			if((jobs_in[i].mode & ~thermo::JOB_PACKED) == 0 && jobs_in[i].check_homo){
				split[i].check_homo = 0;
				thermo::Job h = jobs_in[i]; h.mode = (unsigned char)(2 | (jobs_in[i].mode & thermo::JOB_PACKED));
				homo_of[i] = (uint32_t)split.size();
				split.push_back(h);
			}
		}
	}
	const std::vector<thermo::Job> &jobs = mirror ? jobs_in : split;
	const size_t n_rec = jobs.size(), n_mirror = mirror ? n_in : 0, n = n_rec + n_mirror;
	int rc;
	if((rc = ctx->th_out.ensure(n + 1)) != PCR_OK) return rc;                      // + 1: return_to_host copies whole 16-byte units
	if((rc = ensure_dg_table(ctx, salt)) != PCR_OK) return rc;
	const thermo::Job *d_jobs = nullptr;
	if(n_rec*sizeof(thermo::Job) <= (size_t(16) << 20)){                           // every wave reads its one 72-byte job over the bus
		const void *p = nullptr;
		if((rc = mapped_input(ctx, jobs.data(), n_rec*sizeof(thermo::Job), &p)) != PCR_OK) return rc;
		d_jobs = (const thermo::Job *)p;
	}
	else{
		if((rc = ctx->th_jobs.ensure(n_rec)) != PCR_OK) return rc;
		HIP_TRY(hipMemcpyAsync(ctx->th_jobs.p, jobs.data(), n_rec*sizeof(thermo::Job), hipMemcpyHostToDevice, ctx->stream));
		d_jobs = ctx->th_jobs.p;
	}
	const float log_na = logf(salt);
	{
		ProfScope prof(ctx, PCR_PROF_THERMO);                                      // events around the thermodynamics launch only
		const thermo::ThermoValid plain = { nullptr, nullptr, 0.0f, 0.0f, 0.0f };
		if((rc = launch_thermo(ctx, d_jobs, n_rec, n_mirror, log_na, plain)) != PCR_OK) return rc;
	}
	{
		const uint8_t *back[3];
		if((rc = return_to_host(ctx, ctx->th_out.p, n*sizeof(thermo::JobOut), nullptr, 0, nullptr, 0, back)) != PCR_OK) return rc;
		const thermo::JobOut *res = (const thermo::JobOut *)back[0];
		uint32_t bad = 0;
		for(size_t i = 0;i < n;++i) bad |= res[i].status;
		if(bad & 1u){ g_err = "thermo: internal trace-back error"; return PCR_ERR_RANGE; }
		memcpy(out.data(), res, n_in*sizeof(thermo::JobOut));
		if(mirror){ for(size_t i = 0;i < n_in;++i) out[i].tm_dimer = res[n_in + i].tm_dimer; }
		else{ for(size_t i = 0;i < n_in;++i){ if(homo_of[i] != UINT32_MAX) out[i].tm_dimer = res[homo_of[i]].tm_dimer; } }
	}
	return PCR_OK;
}

// PCR::is_valid without the dimer test for many words at once, degenerate ones included (see thermo::ThermoValid): recs = one
// packed record per word (append_valid_record), n_exp[i] = its number of expansions; bad[i] != 0: some expansion fails.
// st: the stream to work on (default: the handle's).  On another stream the call touches none of the handle's shared staging
// (mapped return buffer, profiling events), so that it may run on a host thread of its own beside work on the handle's stream.
int run_thermo_valid(pcr_ctx *ctx, const std::vector<thermo::Job> &recs, const std::vector<uint32_t> &n_exp, const pcr_thermo_args *a, std::vector<uint8_t> &bad,
	hipStream_t st = nullptr)
{
	const bool aside = st != nullptr && st != ctx->stream;
	if(!st) st = ctx->stream;
	const size_t n_rec = recs.size();
	bad.assign(n_rec, 0);
	if(n_rec == 0) return PCR_OK;
	if(!(a->salt >= 1.0e-6f && a->salt <= 1.0f)){ g_err = "thermo: salt outside [1e-6, 1] (NucCruc::salt, nuc_cruc.h:780-788)"; return PCR_ERR_ARG; }
	size_t n_jobs = 0;
	for(uint32_t e : n_exp) n_jobs += e;
	if(n_jobs >= (size_t(1) << 31)){ g_err = "thermo: too many expansions in one call"; return PCR_ERR_CAPACITY; }
	// jobs in rounds: expansion 0 of every word, then expansion 1 of the degenerate ones, ... -- by the time a word's later
	// expansions come up one of the earlier ones may have failed, and the kernel skips the rest of a word that is already bad
	std::vector<uint2> map(n_jobs);
	{
		std::vector<uint32_t> live(n_rec);
		for(size_t r = 0;r < n_rec;++r) live[r] = (uint32_t)r;
		size_t j = 0, n_live = n_rec;
		for(uint32_t e = 0;n_live;++e){
			size_t keep = 0;
			for(size_t k = 0;k < n_live;++k){
				const uint32_t r = live[k];
				if(e < n_exp[r]){ map[j++] = make_uint2(r, e); live[keep++] = r; }
			}
			n_live = keep;
		}
	}
	int rc;
	if((rc = ctx->th_jobs.ensure(n_rec)) != PCR_OK) return rc;
	if((rc = ctx->th_map.ensure(n_jobs)) != PCR_OK) return rc;
	if((rc = ctx->th_bad.ensure(n_rec + 4)) != PCR_OK) return rc;
	if((rc = ensure_dg_table(ctx, a->salt, st)) != PCR_OK) return rc;
	HIP_TRY(hipMemcpyAsync(ctx->th_jobs.p, recs.data(), n_rec*sizeof(thermo::Job), hipMemcpyHostToDevice, st));
	HIP_TRY(hipMemcpyAsync(ctx->th_map.p, map.data(), n_jobs*sizeof(uint2), hipMemcpyHostToDevice, st));
	HIP_TRY(hipMemsetAsync(ctx->th_bad.p, 0, (n_rec + 4)*sizeof(uint32_t), st));
	{
		ProfScope prof(ctx, PCR_PROF_THERMO, !aside);
		const thermo::ThermoValid V = { ctx->th_map.p, ctx->th_bad.p, a->tm_min, a->tm_max, a->max_hairpin };
		if((rc = launch_thermo(ctx, ctx->th_jobs.p, n_jobs, 0, logf(a->salt), V, st)) != PCR_OK) return rc;
	}
	std::vector<uint32_t> copy;
	const uint32_t *res = nullptr;
	if(aside){
		copy.resize(n_rec);
		HIP_TRY(hipMemcpyAsync(copy.data(), ctx->th_bad.p, n_rec*sizeof(uint32_t), hipMemcpyDeviceToHost, st));
		HIP_TRY(hipStreamSynchronize(st));
		res = copy.data();
	}
	else{
		const uint8_t *back[3];
		if((rc = return_to_host(ctx, ctx->th_bad.p, n_rec*sizeof(uint32_t), nullptr, 0, nullptr, 0, back)) != PCR_OK) return rc;
		res = (const uint32_t *)back[0];
	}
	for(size_t r = 0;r < n_rec;++r){
		if(res[r] & 2u){ g_err = "thermo: internal trace-back error"; return PCR_ERR_RANGE; }
		bad[r] = (uint8_t)(res[r] & 1u);
	}
	return PCR_OK;
}

const size_t MAX_EXPANSIONS = 1u << 16;

// One packed record for the word and its number of expansions (PCR::is_valid's strand = primer_strand / degeneracy,
// valid_pcr.cpp:13); false: holes between the oligo's ends, longer than 32, or more than MAX_EXPANSIONS expansions.
bool append_valid_record(const Planes &w, const pcr_thermo_args *args, std::vector<thermo::Job> &recs, std::vector<uint32_t> &n_exp)
{
	const uint32_t occ = pcrhost::planes_occupied(w);
	if(!occ) return false;
	const int first = __builtin_ctz(occ), len = 32 - __builtin_clz(occ) - first;
	if(len > (int)thermo::MAXL || __builtin_popcount(occ) != len) return false;
	const double degen = pcrhost::planes_degeneracy(w);
	if(degen > (double)MAX_EXPANSIONS) return false;
	thermo::Job j; memset(&j, 0, sizeof(j));
	const uint32_t pl[4] = {w.a, w.c, w.g, w.t};
	memcpy(j.q, pl, sizeof(pl));
	j.t[0] = (unsigned char)first; j.qlen = (unsigned char)len; j.mode = thermo::JOB_PACKED;
	j.log_strand = logf((float)(args->primer_strand/degen));
	recs.push_back(j);
	n_exp.push_back((uint32_t)degen);
	return true;
}

// A plain oligo (one base per slot, no hole between its ends) goes straight from its bit planes to codes:
// the common case of every caller, and the IUPAC expansion below is vectors of vectors.
inline bool plain_oligo_codes(const Planes &w, unsigned char *dst, unsigned char &len)
{
	const uint32_t occ = pcrhost::planes_occupied(w);
	if(!occ) return false;
	const int first = __builtin_ctz(occ), last = 31 - __builtin_clz(occ);
	const int n = last - first + 1;
	if(n > (int)thermo::MAXL || __builtin_popcount(occ) != n) return false;
	if(__builtin_popcount(w.a) + __builtin_popcount(w.c) + __builtin_popcount(w.g) + __builtin_popcount(w.t) != n) return false;
	for(int k = 0;k < n;++k){
		const int b = first + k;
		dst[k] = (unsigned char)(((w.c >> b) & 1) | (((w.g >> b) & 1) << 1) | (((w.t >> b) & 1)*3));
	}
	len = (unsigned char)n;
	return true;
}

// The jobs of PCR::is_valid for one oligo (every IUPAC expansion at strand/degeneracy, valid_pcr.cpp:9-13).
bool append_valid_jobs(const Planes &w, const pcr_thermo_args *args, int check_homo, std::vector<thermo::Job> &jobs)
{
	thermo::Job j; memset(&j, 0, sizeof(j));
	j.mode = 0; j.check_homo = check_homo ? 1 : 0;
	{
		// a plain oligo travels as its four slot masks; the kernel spells the codes (the host loop over the slots was most of
		// pcr_thermo's time at 20 000 oligos)
		const uint32_t occ = pcrhost::planes_occupied(w);
		const int first = occ ? __builtin_ctz(occ) : 0, len = occ ? 32 - __builtin_clz(occ) - first : 0;
		if(occ && len <= (int)thermo::MAXL && __builtin_popcount(occ) == len
			&& __builtin_popcount(w.a) + __builtin_popcount(w.c) + __builtin_popcount(w.g) + __builtin_popcount(w.t) == len){
			const uint32_t pl[4] = {w.a, w.c, w.g, w.t};
			memcpy(j.q, pl, sizeof(pl));
			j.t[0] = (unsigned char)first; j.qlen = (unsigned char)len; j.mode = thermo::JOB_PACKED;
			// (the same strand for every plain oligo of a call: one logf instead of one per oligo)
			static thread_local float memo_in = -1.0f, memo_out = 0.0f;
			const float strand1 = (float)(args->primer_strand/1.0);
			if(strand1 != memo_in){ memo_in = strand1; memo_out = logf(strand1); }
			j.log_strand = memo_out;
			jobs.push_back(j);
			return true;
		}
	}
	const double degen = pcrhost::planes_degeneracy(w);
	if(degen > (double)MAX_EXPANSIONS) return false;
	const float strand = (float)(args->primer_strand/degen);                       // valid_pcr.cpp:13
	j.log_strand = logf(strand);
	bool ok = true; size_t n = 0;
	const bool done = pcrhost::for_each_expansion(w, MAX_EXPANSIONS, [&](const uint8_t *b, int len){
		if(len < 1 || len > (int)thermo::MAXL){ ok = false; return; }
		for(int i = 0;i < len;++i){ if(b[i] > 3) ok = false; j.q[i] = b[i]; }
		j.qlen = (unsigned char)len;
		jobs.push_back(j); ++n;
	});
	return done && ok && n > 0;
}

// The jobs of PCR::max_dimer_tm for one pair (pcr_assay.cpp:232-269).
bool append_dimer_jobs(const Planes &F, const Planes &R, const pcr_thermo_args *args, std::vector<thermo::Job> &jobs)
{
	thermo::Job j; memset(&j, 0, sizeof(j));
	j.mode = 1;
	if(plain_oligo_codes(F, j.q, j.qlen) && plain_oligo_codes(R, j.t, j.tlen)){
		const float c = (float)(args->primer_strand/1.0);
		j.log_strand = logf(c - 0.5f*c);                                         // nuc_cruc.h:832-837 with equal concentrations
		jobs.push_back(j);
		return true;
	}
	std::vector<std::vector<uint8_t> > ef, er;
	if(!pcrhost::expand_oligo(F, ef, MAX_EXPANSIONS) || !pcrhost::expand_oligo(R, er, MAX_EXPANSIONS) || ef.size()*er.size() > MAX_EXPANSIONS) return false;
	const float ca = (float)(args->primer_strand/pcrhost::planes_degeneracy(F));      // pcr_assay.cpp:244
	const float cb = (float)(args->primer_strand/pcrhost::planes_degeneracy(R));
	const float strand = (ca > cb) ? ca - 0.5f*cb : cb - 0.5f*ca;                // nuc_cruc.h:832-837
	j.log_strand = logf(strand);
	for(const std::vector<uint8_t> &f : ef) for(const std::vector<uint8_t> &r : er){
		if(!job_set(j.q, j.qlen, f) || !job_set(j.t, j.tlen, r)) return false;
		jobs.push_back(j);
	}
	return true;
}

} // namespace

extern "C" {

int pcr_thermo(pcr_ctx *ctx, const pcr_word128 *oligos, uint32_t n, int check_homo_dimer, const pcr_thermo_args *args,
	pcr_thermo_result *out)
{
	if(!ctx || !args || (n && (!oligos || !out))){ g_err = "pcr_thermo: bad argument"; return PCR_ERR_ARG; }
	FLUSH(ctx);
	HIP_TRY(hipSetDevice(ctx->device));
	std::vector<thermo::Job> &jobs = ctx->th_host_jobs;                          // (the handle's: a fresh 1.4 MB vector per call of 20 000 oligos is page faults)
	jobs.clear();
	jobs.reserve(n);
	std::vector<uint32_t> first(n + 1, 0);
	for(uint32_t i = 0;i < n;++i){
		first[i] = (uint32_t)jobs.size();
		const Planes w = pcrhost::planes_of_word(oligos[i].w);
		if(!pcrhost::planes_occupied(w)){ g_err = "pcr_thermo: empty oligo"; return PCR_ERR_ARG; }
		if(!append_valid_jobs(w, args, check_homo_dimer, jobs)){
			g_err = "pcr_thermo: oligo is longer than 32, holds a non-base slot (NucCruc::set_query throws) or has more than 65536 expansions";
			return (pcrhost::planes_degeneracy(w) > (double)MAX_EXPANSIONS) ? PCR_ERR_CAPACITY : PCR_ERR_ARG;
		}
	}
	first[n] = (uint32_t)jobs.size();
	std::vector<thermo::JobOut> &res = ctx->th_host_res;
	int rc = run_thermo_jobs(ctx, jobs, args->salt, res);
	if(rc != PCR_OK) return rc;
	for(uint32_t i = 0;i < n;++i){
		pcr_thermo_result r; memset(&r, 0, sizeof(r));
		r.n_expansions = first[i + 1] - first[i];
		r.valid = 1;
		for(uint32_t k = first[i];k < first[i + 1];++k){ if(!thermo_expansion_valid(res[k], *args, check_homo_dimer)) r.valid = 0; }
		if(r.n_expansions){
			const thermo::JobOut &o = res[first[i]];
			r.tm = o.tm_pm; r.dH = o.dH_pm; r.dS = o.dS_pm; r.hairpin_tm = o.tm_hairpin; r.homodimer_tm = o.tm_dimer;
			r.dG = thermo_delta_g(o);
		}
		out[i] = r;
	}
	return PCR_OK;
}

// The validity form (thermo::ThermoValid) as the local search drives it (pcr_optimize.inc: one record per trial word, then
// run_thermo_valid), for a caller's own words.
int pcr_valid_words(pcr_ctx *ctx, const pcr_word128 *words, uint32_t n, const pcr_thermo_args *args, uint8_t *valid_out)
{
	if(!ctx || !args || (n && (!words || !valid_out))){ g_err = "pcr_valid_words: bad argument"; return PCR_ERR_ARG; }
	FLUSH(ctx);
	HIP_TRY(hipSetDevice(ctx->device));
	std::vector<thermo::Job> recs;
	std::vector<uint32_t> n_exp;
	recs.reserve(n); n_exp.reserve(n);
	for(uint32_t i = 0;i < n;++i){
		const Planes w = pcrhost::planes_of_word(words[i].w);
		if(!pcrhost::planes_occupied(w)){ g_err = "pcr_valid_words: empty oligo"; return PCR_ERR_ARG; }
		if(!append_valid_record(w, args, recs, n_exp)){
			g_err = "pcr_valid_words: oligo is longer than 32, holds a non-base slot (NucCruc::set_query throws) or has more than 65536 expansions";
			return (pcrhost::planes_degeneracy(w) > (double)MAX_EXPANSIONS) ? PCR_ERR_CAPACITY : PCR_ERR_ARG;
		}
	}
	std::vector<uint8_t> bad;
	const int rc = run_thermo_valid(ctx, recs, n_exp, args, bad);
	if(rc != PCR_OK) return rc;
	for(uint32_t i = 0;i < n;++i) valid_out[i] = bad[i] ? 0 : 1;
	return PCR_OK;
}

int pcr_dimer(pcr_ctx *ctx, const pcr_pair *pairs, uint32_t n, const pcr_thermo_args *args, float *max_tm)
{
	if(!ctx || !args || (n && (!pairs || !max_tm))){ g_err = "pcr_dimer: bad argument"; return PCR_ERR_ARG; }
	FLUSH(ctx);
	HIP_TRY(hipSetDevice(ctx->device));
	std::vector<thermo::Job> jobs;
	jobs.reserve(n);
	std::vector<uint32_t> first(n + 1, 0);
	for(uint32_t i = 0;i < n;++i){
		first[i] = (uint32_t)jobs.size();
		const Planes F = pcrhost::planes_of_word(pairs[i].f.w), R = pcrhost::planes_of_word(pairs[i].r.w);
		if(!append_dimer_jobs(F, R, args, jobs)){
			g_err = "pcr_dimer: bad oligo or too many expansions";
			return (pcrhost::planes_degeneracy(F)*pcrhost::planes_degeneracy(R) > (double)MAX_EXPANSIONS) ? PCR_ERR_CAPACITY : PCR_ERR_ARG;
		}
	}
	first[n] = (uint32_t)jobs.size();
	std::vector<thermo::JobOut> res;
	int rc = run_thermo_jobs(ctx, jobs, args->salt, res);
	if(rc != PCR_OK) return rc;
	for(uint32_t i = 0;i < n;++i){
		float m = 0.0f;
		for(uint32_t k = first[i];k < first[i + 1];++k) m = std::max(m, res[k].tm_dimer);   // :262
		max_tm[i] = m;
	}
	return PCR_OK;
}

int pcr_multiplex_compatible(pcr_ctx *ctx, const pcr_pair *a, const pcr_pair *b, uint32_t n, const pcr_thermo_args *args, uint8_t *ok)
{
	if(!ctx || !args || (n && (!a || !b || !ok))){ g_err = "pcr_multiplex_compatible: bad argument"; return PCR_ERR_ARG; }
	FLUSH(ctx);
	HIP_TRY(hipSetDevice(ctx->device));
	std::vector<thermo::Job> jobs;
	std::vector<uint32_t> first(n + 1, 0);
	const float log_strand = logf(args->primer_strand);                          // pcr_assay.cpp:819-821
	for(uint32_t i = 0;i < n;++i){
		first[i] = (uint32_t)jobs.size();
		const uint64_t *qa[2] = {a[i].f.w, a[i].r.w}, *sb[2] = {b[i].f.w, b[i].r.w};
		for(int qo = 0;qo < 2;++qo){
			std::vector<std::vector<uint8_t> > eq;
			if(!pcrhost::expand_oligo(pcrhost::planes_of_word(qa[qo]), eq, MAX_EXPANSIONS)){ g_err = "too many expansions"; return PCR_ERR_CAPACITY; }
			for(int so = 0;so < 2;++so){
				std::vector<std::vector<uint8_t> > es;
				if(!pcrhost::expand_oligo(pcrhost::planes_of_word(sb[so]), es, MAX_EXPANSIONS) || eq.size()*es.size() > MAX_EXPANSIONS){
					g_err = "too many expansions"; return PCR_ERR_CAPACITY;
				}
				for(const std::vector<uint8_t> &q : eq) for(const std::vector<uint8_t> &s : es){
					thermo::Job j; memset(&j, 0, sizeof(j));
					if(!job_set(j.q, j.qlen, q) || !job_set(j.t, j.tlen, s)){ g_err = "pcr_multiplex_compatible: bad oligo"; return PCR_ERR_ARG; }
					j.mode = 1; j.log_strand = log_strand;
					jobs.push_back(j);
				}
			}
		}
	}
	first[n] = (uint32_t)jobs.size();
	std::vector<thermo::JobOut> res;
	int rc = run_thermo_jobs(ctx, jobs, args->salt, res);
	if(rc != PCR_OK) return rc;
	for(uint32_t i = 0;i < n;++i){
		uint8_t good = 1;
		for(uint32_t k = first[i];k < first[i + 1];++k){ if(res[k].tm_dimer >= args->max_dimer) good = 0; }   // :841
		ok[i] = good;
	}
	return PCR_OK;
}

} // extern "C"

#include "pcr_sampler.inc"
#include "pcr_multiplex.inc"
#include "pcr_optimize.inc"
