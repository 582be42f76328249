// pcr_select_sites (included by pcr_device.hip after pcr_select.inc): the set's word DB filled with EVERY entry Sequence::pack
// emits that some oligo of the batch matches at or above its floor -- pack + match_words, as the reference fills the multiplex
// DB (main.cpp:989-1001) -- instead of select_words' arg-max per (oligo, sequence).
//
// The counting is the bit-sliced counter of pcr_scan_bitsliced.inc (same tables, same launch geometry); the hit path differs.
// An all-sites pass keeps every hit, at thresholds 0.5 - 0.8 that is orders of magnitude more than the arg-max pass records,
// and the lanes of a wave are consecutive windows of one sequence: so there is no best[], a window contributes at most one
// hit per strand (whichever oligos match it: the DB entry is the window, the union over oligos is taken here instead of by
// the sort), and a wave appends its hits with ONE atomicAdd on the sequence's fill.

namespace {

struct SitesSlow { const uint4 *cand_fwd, *cand_rc; const uint32_t *cand_floor; uint32_t ncand; uint32_t pad; };

// Exact recount (plane popcount) of the orientations the counter flagged in one word, for a window whose planes the caller
// holds.  Orientation o_base + j = 2*candidate + strand with o_base a multiple of 32: even bits are the oligos as stored
// (plus-strand word), odd bits their reverse complements (minus-strand word).  -> bit 0: a plus-strand match, bit 1: a minus.
// `have` (strands already found) spares the recounts that could not add anything.  Out of line, arguments in LDS: see Scan2Slow.
__device__ __noinline__ uint32_t sites_recount(uint32_t bits, uint32_t o_base, uint32_t have, uint32_t wa, uint32_t wc, uint32_t wg, uint32_t wt,
	const SitesSlow *A)
{
	if(have & 1u) bits &= 0xAAAAAAAAu;
	if(have & 2u) bits &= 0x55555555u;
	const uint32_t ncand = A->ncand;
	while(bits){
		const uint32_t j = __ffs(bits) - 1;
		bits &= bits - 1;
		const uint32_t o = o_base + j, c = o >> 1;
		if(c >= ncand) continue;
		const uint32_t cnt = match_count(wa, wc, wg, wt, (o & 1u) ? A->cand_rc[c] : A->cand_fwd[c]);
		if(cnt >= A->cand_floor[c]){
			have |= 1u << (o & 1u);
			bits &= (o & 1u) ? 0x55555555u : 0xAAAAAAAAu;           // the strand is settled
		}
	}
	return have;
}

// grid.x = tiles, grid.y = orientation groups of this launch (group index = group0 + blockIdx.y); tables as k_scan2, the
// orientations on the counter bits in their own order (bit b of the pass = orientation b).
template<int NW, int NSLOT, int KLO>
__global__ __launch_bounds__(SCAN2_THREADS) void k_scan_sites(
	const uint32_t *__restrict__ nib, const uint4 *__restrict__ planes, const uint32_t *__restrict__ valid,
	const uint64_t *__restrict__ blk_off, const uint64_t *__restrict__ len, const uint8_t *__restrict__ active,
	const uint32_t *__restrict__ tile_seq, const uint32_t *__restrict__ tile_pos0,
	const uint32_t *__restrict__ tab, const uint32_t *__restrict__ bias, uint32_t group0, uint32_t group_words,
	const uint4 *__restrict__ cand_fwd, const uint4 *__restrict__ cand_rc, const uint32_t *__restrict__ cand_floor,
	uint32_t ncand, Hit *__restrict__ hits, uint32_t *__restrict__ seq_count, uint32_t *__restrict__ counters, uint32_t cap)
{
	static_assert(NSLOT % 2 == 0 && KLO + NSLOT <= 32, "slot range");
	__shared__ __attribute__((aligned(16))) uint32_t lds_tab[NSLOT*16*8];
	__shared__ SitesSlow slow_args;
	const uint32_t tile = blockIdx.x;
	const uint32_t seq = tile_seq[tile];
	if(!active[seq]) return;
	if(threadIdx.x == 0){
		slow_args.cand_fwd = cand_fwd; slow_args.cand_rc = cand_rc; slow_args.cand_floor = cand_floor; slow_args.ncand = ncand; slow_args.pad = 0;
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
	const uint32_t lane = threadIdx.x & 63u;

#pragma unroll 1
	for(int i = 0;i < SCAN2_NPOS;++i){
		const uint32_t p = p0 + threadIdx.x + SCAN2_THREADS*i;
		uint32_t strands = 0;                                       // bit 0: the window matches as a plus-strand word, bit 1: as a minus-strand word
		if((uint64_t)p + 32 <= L){
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

			// (`s` is never indexed dynamically: see k_scan2)
			uint32_t any = 0;
#pragma unroll
			for(int w = 0;w < NW;++w) any |= s.hi.v[w];
			const uint32_t b = p >> 5, sh = p & 31;
			if(any && ((valid[base + b] >> sh) & 1u)){               // pack's filters, as scan2_slow_path checks them
				const uint4 lo = planes[base + b];
				const uint4 hi4 = planes[base + b + 1];
				const uint32_t wa = funnel(lo.x, hi4.x, sh), wc = funnel(lo.y, hi4.y, sh);
				const uint32_t wg = funnel(lo.z, hi4.z, sh), wt = funnel(lo.w, hi4.w, sh);
#pragma unroll
				for(int w = 0;w < NW;++w){
					if(s.hi.v[w] && strands != 3u) strands = sites_recount(s.hi.v[w], (group*group_words + w)*32, strands, wa, wc, wg, wt, &slow_args);
				}
			}
		}
		// the wave's hits of this batch of 64 windows: one atomicAdd on the sequence's fill, slots by lane rank (plus before minus)
		const uint64_t m_plus = __ballot(strands & 1u), m_minus = __ballot(strands & 2u);
		if(m_plus | m_minus){
			const uint32_t total = (uint32_t)(__builtin_popcountll(m_plus) + __builtin_popcountll(m_minus));
			const uint32_t leader = (uint32_t)__builtin_ctzll(m_plus | m_minus);
			uint32_t first = 0;
			if(lane == leader){
				first = atomicAdd(&seq_count[seq], total);
				if(first + total > cap){ atomicOr(&counters[0], 1u); atomicMax(&counters[2], first + total); }
			}
			first = __shfl(first, leader);
			const uint64_t below = (1ull << lane) - 1ull;
			uint32_t slot = first + (uint32_t)(__builtin_popcountll(m_plus & below) + __builtin_popcountll(m_minus & below));
			if(strands & 1u){
				if(slot < cap){ Hit h; h.key = make_key(seq, (int32_t)p, 1, 0, 0); h.cand = 0; h.cnt = 0; hits[(size_t)seq*cap + slot] = h; }   // sequence.cpp:184
				++slot;
			}
			if((strands & 2u) && slot < cap){ Hit h; h.key = make_key(seq, (int32_t)p + 31, 2, 0, 0); h.cand = 0; h.cnt = 0; hits[(size_t)seq*cap + slot] = h; }   // sequence.cpp:190
		}
	}
}

// The irregular words: scan_irr_block without best[] -- a word is appended once, whichever oligos match it.  Words of one
// wave belong to many sequences, so each hit takes its own slot.
__global__ __launch_bounds__(IRR_THREADS) void k_scan_irr_sites(const IrrDev *__restrict__ irr, const uint32_t *__restrict__ perm, uint32_t n_live,
	const uint8_t *__restrict__ active, const uint4 *__restrict__ cand_fwd, const uint32_t *__restrict__ cand_floor, uint32_t ncand,
	Hit *__restrict__ hits, uint32_t *__restrict__ seq_count, uint32_t *__restrict__ counters, uint32_t cap)
{
	uint32_t wa[IRR_PER_LANE], wc[IRR_PER_LANE], wg[IRR_PER_LANE], wt[IRR_PER_LANE];
	bool hit[IRR_PER_LANE];
	const uint32_t i0 = blockIdx.x*(IRR_THREADS*IRR_PER_LANE) + threadIdx.x;
#pragma unroll
	for(int k = 0;k < IRR_PER_LANE;++k){
		const uint32_t i = i0 + k*IRR_THREADS;
		wa[k] = wc[k] = wg[k] = wt[k] = 0; hit[k] = false;     // an empty word matches nothing
		if(i < n_live){
			const IrrDev e = irr[perm[i]];
			if(active[e.seq]){ wa[k] = e.w.a; wc[k] = e.w.c; wg[k] = e.w.g; wt[k] = e.w.t; }
		}
	}
#pragma unroll 8
	for(uint32_t c = 0;c < ncand;++c){
		const uint4 m = cand_fwd[c];
		const uint32_t fl = max(cand_floor[c], 1u);          // floor 0 ("everything matches") still needs the word to exist
		const bool zero_floor = cand_floor[c] == 0;
#pragma unroll
		for(int k = 0;k < IRR_PER_LANE;++k){
			const uint32_t cnt = match_count(wa[k], wc[k], wg[k], wt[k], m);
			hit[k] = hit[k] || cnt >= fl || (zero_floor && (wa[k] | wc[k] | wg[k] | wt[k]));
		}
	}
#pragma unroll
	for(int k = 0;k < IRR_PER_LANE;++k){
		if(!hit[k]) continue;                                 // (a hit implies i < n_live: the other lanes hold empty words)
		const IrrDev e = irr[perm[i0 + k*IRR_THREADS]];
		const uint32_t slot = atomicAdd(&seq_count[e.seq], 1u);
		if(slot < cap){
			Hit h; h.key = make_key(e.seq, e.loc, e.meta & 0xFF, 1, (e.meta >> 16) & 0xFF); h.cand = 0; h.cnt = 0;
			hits[(size_t)e.seq*cap + slot] = h;
		}
		else{ atomicOr(&counters[0], 1u); atomicMax(&counters[2], slot + 1); }
	}
}

template<int NSLOT, int KLO>
int launch_scan_sites_nw(pcr_ctx *ctx, SeqSet &S, uint32_t nw, uint32_t group0, uint32_t n_groups, uint32_t gw, const HitSink &sink,
	const uint32_t *d_tab, const uint32_t *d_bias)
{
#define SITES_ARGS S.nib.p, S.planes.p, S.valid_d(), S.d_blk_off.p, S.d_len.p, S.d_active.p, S.tile_seq.p, S.tile_pos0.p, \
	d_tab, d_bias, group0, gw, ctx->d_cand_fwd, ctx->d_cand_rc, ctx->d_cand_floor, sink.ncand, sink.hits, sink.seq_count, sink.counters, sink.cap
	const dim3 grid(S.n_tiles, n_groups), block(SCAN2_THREADS);
	switch(nw){
		case 1: hipLaunchKernelGGL((k_scan_sites<1, NSLOT, KLO>), grid, block, 0, ctx->stream, SITES_ARGS); break;
		case 2: hipLaunchKernelGGL((k_scan_sites<2, NSLOT, KLO>), grid, block, 0, ctx->stream, SITES_ARGS); break;
		case 3: hipLaunchKernelGGL((k_scan_sites<3, NSLOT, KLO>), grid, block, 0, ctx->stream, SITES_ARGS); break;
		case 4: hipLaunchKernelGGL((k_scan_sites<4, NSLOT, KLO>), grid, block, 0, ctx->stream, SITES_ARGS); break;
		case 5: hipLaunchKernelGGL((k_scan_sites<5, NSLOT, KLO>), grid, block, 0, ctx->stream, SITES_ARGS); break;
		case 6: hipLaunchKernelGGL((k_scan_sites<6, NSLOT, KLO>), grid, block, 0, ctx->stream, SITES_ARGS); break;
		case 7: hipLaunchKernelGGL((k_scan_sites<7, NSLOT, KLO>), grid, block, 0, ctx->stream, SITES_ARGS); break;
		default: hipLaunchKernelGGL((k_scan_sites<8, NSLOT, KLO>), grid, block, 0, ctx->stream, SITES_ARGS); break;
	}
#undef SITES_ARGS
	HIP_TRY(hipGetLastError());
	return PCR_OK;
}

// Full groups (8 counter words) in one launch, the partial last group in a second one (as launch_scan2), then the irregular words.
int launch_sites(pcr_ctx *ctx, SeqSet &S, const ScanPlan &P, const Scan2Staged &B, const HitSink &sink)
{
	int rc = PCR_OK;
	const Scan2Tables &T = B.T;
	if(S.n_tiles && T.n_groups){
		ProfScope scan_prof(ctx, PCR_PROF_SCAN, ctx->prof && (ctx->prof_pass++ % ctx->prof_stride) == 0);
		const uint32_t full = (T.last_words == T.gw) ? T.n_groups : T.n_groups - 1;
		if(full){
			rc = (T.nslot == 26) ? launch_scan_sites_nw<26, 3>(ctx, S, T.gw, 0, full, T.gw, sink, B.d_tab, B.d_bias)
				: launch_scan_sites_nw<32, 0>(ctx, S, T.gw, 0, full, T.gw, sink, B.d_tab, B.d_bias);
			if(rc != PCR_OK) return rc;
		}
		if(full < T.n_groups){
			rc = (T.nslot == 26) ? launch_scan_sites_nw<26, 3>(ctx, S, T.last_words, full, 1, T.gw, sink, B.d_tab, B.d_bias)
				: launch_scan_sites_nw<32, 0>(ctx, S, T.last_words, full, 1, T.gw, sink, B.d_tab, B.d_bias);
			if(rc != PCR_OK) return rc;
		}
		scan_prof.finish();
	}
	if(P.n_live){
		const unsigned irr_grid = (P.n_live + IRR_THREADS*IRR_PER_LANE - 1)/(IRR_THREADS*IRR_PER_LANE);
		hipLaunchKernelGGL(k_scan_irr_sites, dim3(irr_grid), dim3(IRR_THREADS), 0, ctx->stream, S.irr.p, S.irr_perm.p, P.n_live,
			S.d_active.p, ctx->d_cand_fwd, ctx->d_cand_floor, sink.ncand, sink.hits, sink.seq_count, sink.counters, sink.cap);
		HIP_TRY(hipGetLastError());
	}
	return rc;
}

// pcr_select_sites proper (arguments checked by the caller).  Always the bit-sliced form: the seed scans record their hits
// through best[].  best[] and the pass epoch are neither allocated nor touched, so a later pcr_select_words finds them as its
// last pass left them.
int select_sites_impl(pcr_ctx *ctx, pcr_set which, const pcr_pair *pairs, uint32_t n_pairs, float threshold, uint32_t min_oligo_length,
	uint64_t *n_entries_out)
{
	HIP_TRY(hipSetDevice(ctx->device));
	SeqSet &S = ctx->sets[which];
	S.have_db = false; S.n_entries = 0;
	if(n_entries_out) *n_entries_out = 0;
	S.ctrl_clean = false; S.touched_from_seg = false;
	HostTimer timer(ctx, 0);
	if(ctx->timing) ++ctx->n_timed;
	PassJob J;
	std::vector<pcrhost::Candidate> &cand = J.cand;
	pcrhost::build_candidates((const uint64_t *)pairs, n_pairs, false, false, threshold, cand);
	const uint32_t ncand = (uint32_t)cand.size();
	if(S.n == 0 || ncand == 0){ S.have_db = true; S.n_touched = 0; return PCR_OK; }
	int rc;
	ScanPlan &P = J.P;
	P.form = ScanForm::BitSliced; P.need_plain = true;
	P.min_len = min_oligo_length; P.n_live = live_irregular(S, min_oligo_length);
	P.or_plain.resize(2*(size_t)ncand);
	for(uint32_t o = 0;o < 2*ncand;++o) P.or_plain[o] = o;      // bit b = orientation b: sites_recount relies on it
	if(ctx->debug_log) fprintf(stderr, "[pcramp] all-sites plan: %u candidates, %u/%u IUPAC tiles, %u live irregular words, %u-slot buckets\n",
		ncand, S.n_degen_tiles, S.n_tiles, P.n_live, S.bucket_cap);
	StagedTables T;
	prepare_tables(S, J, nullptr);
	timer.next(1);
	if((rc = stage_tables(ctx, S, J, nullptr, false, false, T)) != PCR_OK) return rc;

	timer.next(2);
	uint32_t h_counters[4];
	if((rc = S.touched.ensure(S.n)) != PCR_OK) return rc;
	S.d_seg_hi = S.ctrl.p + 8 + S.n;
	for(int attempt = 0;;++attempt){
		const uint32_t cap = S.bucket_cap;
		const uint64_t n_slots = (uint64_t)S.n*cap;
		if(n_slots >= (uint64_t(1) << 32) || n_slots*(sizeof(Hit) + sizeof(DevEntry)) > (uint64_t(96) << 30)){
			S.bucket_cap = 64;
			g_err = "pcr_select_sites: the per-sequence hit buckets would not fit (too many sites per sequence)"; return PCR_ERR_CAPACITY;
		}
		if((rc = ctx->hits.ensure(n_slots)) != PCR_OK) return rc;
		if((rc = S.db.ensure(n_slots)) != PCR_OK) return rc;
		if(attempt > 0) HIP_TRY(hipMemsetAsync(S.ctrl.p, 0, (8 + 2*(size_t)S.n)*sizeof(uint32_t), ctx->stream));
		HitSink sink; sink.best = nullptr; sink.hits = ctx->hits.p; sink.seq_count = S.ctrl.p + 8;
		sink.counters = S.ctrl.p; sink.cap = cap; sink.ncand = ncand; sink.epoch = 0;
		if((rc = launch_sites(ctx, S, P, T.plain, sink)) != PCR_OK) return rc;
		if((rc = plain_tail<true>(ctx, S, sink, false, nullptr)) != PCR_OK) return rc;
		timer.next(3);
		if((rc = mail_wait(ctx, ctx->mail_seq, h_counters)) != PCR_OK) return rc;
		timer.next(2);
		S.db_cap = cap; S.n_slots = n_slots;
		const bool overflowed = (h_counters[0] & 1u) != 0;
		if(overflowed && (attempt >= 12 || cap >= MAX_BUCKET_CAP_GLOBAL)){
			S.bucket_cap = 64;
			g_err = "pcr_select_sites: more than 65536 candidate sites in one sequence (per-sequence bucket limit)"; return PCR_ERR_CAPACITY;
		}
		const uint32_t want = resized_buckets(overflowed, cap, h_counters[2], attempt);
		if(!want) break;
		S.bucket_cap = want;
	}
	if(ctx->debug_log) fprintf(stderr, "[pcramp] all-sites pass done: %u-slot buckets, largest fill %u, %u sequences with entries\n", S.db_cap, h_counters[2], h_counters[3]);
	S.n_touched = h_counters[3];
	S.n_entries = S.n_touched ? 1 : 0;
	S.have_db = true;
	if(n_entries_out){
		if((rc = count_entries(ctx, S)) != PCR_OK) return rc;
		*n_entries_out = S.n_entries;
	}
	return PCR_OK;
}

} // namespace

extern "C" int pcr_select_sites(pcr_ctx *ctx, pcr_set which, const pcr_pair *pairs, uint32_t n_pairs, float threshold, uint32_t min_oligo_length,
	uint64_t *n_entries_out)
{
	if(!set_ok(which)){ g_err = "pcr_select_sites: unknown sequence set"; return PCR_ERR_ARG; }
	if(which == PCR_SET_MULTIPLEX){ g_err = "pcr_select_sites: PCR_SET_MULTIPLEX is not supported (PCR_SET_TARGET or PCR_SET_BACKGROUND)"; return PCR_ERR_ARG; }
	if(min_oligo_length < 1 || min_oligo_length > 32){ g_err = "pcr_select_sites: min_oligo_length must be in [1,32]"; return PCR_ERR_ARG; }
	if(!ctx || (n_pairs && !pairs)){ g_err = "pcr_select_sites: bad argument"; return PCR_ERR_ARG; }
	DRAIN(ctx);
	return select_sites_impl(ctx, which, pairs, n_pairs, threshold, min_oligo_length, n_entries_out);
}
