// Per-site duplex Tm (pcr_site_tm; included by pcr_device.hip after pcr_pool.inc, whose item stage it runs).  The melting entry
// points built on the same items share two things of this file: site_oligo / site_oligo_table, the distinct-oligo table with
// its refusals, and melt_items, the melt stage (the only place k_site_tm is launched from).
//
// For every distinct oligo of a panel and every site of the word DB it matches at threshold^2: where the site is, how many
// slots match, and NucCruc's heterodimer Tm / dH / dS of the oligo against the template strand it anneals to there -- the
// definition is written out at pcr_site_tm in include/pcramp_hip.h.  Nothing but the device-resident DB is read:
//   1. item_count / item_fill (pcr_pool.inc): the (entry, oligo) items, one per (oligo, site).  Their number is the record
//      count; a count-only call (or one whose cap is too small) ends between the two.
//   2. melt_items: k_site_jobs + a scan, item k gets n_expansions[oligo] consecutive jobs; then
//   3. k_site_tm: one wave per (item, expansion), grid-strided, THERMO_WAVES independent waves per block around one LDS copy of
//      the dG table -- k_thermo_wave's shape, because the per-wave slab (thermo::WaveSlab, 11.6 KB) is the Engine's and 12 of
//      them plus the table are what 160 KB of LDS hold.  The wave finds its item by bisection of the job offsets, picks the
//      entry the target is read from, spells the query from the oligo's slot masks and the expansion index and the target from
//      the entry's planes, and runs Engine<1>::fill_wave -> collect_rows -> enumerate_parallel<false>.  No thermo::Job exists.
//   4. Two radix sorts put the items into (oligo, sequence, loc5, strand) order; k_site_reduce, a thread per record, walks the
//      item's expansions in index order (max, min, lowest index on a tie: no float atomics) and writes the record in place.
// The call owns its scratch (pcr_ctx::site_*); the dG table is the handle's (th_dg, keyed by its salt as for every thermo call).

namespace {

constexpr int SITE_WAVES = thermo::THERMO_WAVES;
constexpr int SITE_THREADS = 64*SITE_WAVES;
constexpr size_t SITE_LDS = thermo::THERMO_LDS;
constexpr uint32_t SITE_ST_ERROR = 1u, SITE_ST_NO_TM = 2u;                     // bits of a job's status word

struct SiteOligoX { uint32_t n_exp; float log_strand; };                        // beside PoolOligo: expansions, log of the two-strand concentration

__device__ __forceinline__ uint32_t planes_occ(const Planes &w) { return w.a | w.c | w.g | w.t; }

// T: the oligo's slots and one flanking slot on either side, clipped to the word
__device__ __forceinline__ uint32_t site_window(int32_t start, int32_t stop)
{
	const int lo = max(start - 1, 0), hi = min(stop + 1, 31);
	const uint32_t upto = (hi >= 31) ? 0xFFFFFFFFu : ((1u << (hi + 1)) - 1u);
	return upto & ~((1u << lo) - 1u);
}

__device__ __forceinline__ bool planes_less(const Planes &x, const Planes &y)
{
	if(x.a != y.a) return x.a < y.a;
	if(x.c != y.c) return x.c < y.c;
	if(x.g != y.g) return x.g < y.g;
	return x.t < y.t;
}

// The entry a site's target is read from: among the entries sharing (loc, strand) with db[slot] -- the first of them that
// matches the oligo, which is where k_pool_entry_oligos lists the item -- and matching it, the one with the most occupied
// slots in T; on a tie the lowest slot masks.  Entries of a segment are sorted by (loc, strand, ...): the sharers follow.
__device__ __forceinline__ DevEntry site_pick(const DevEntry *__restrict__ db, uint32_t slot, uint32_t seg_end, const PoolOligo &o, uint32_t T)
{
	DevEntry best = db[slot];
	const uint4 m = make_uint4(o.m.a, o.m.c, o.m.g, o.m.t);
	const int32_t loc = best.loc; const uint32_t strand = best.strand;
	int most = __popc(planes_occ(best.w) & T);
	for(uint32_t p = slot + 1;p < seg_end;++p){
		const DevEntry q = db[p];
		if(q.loc != loc || q.strand != strand) break;
		if(!pool_hit(q.w, m, o.floor2)) continue;
		const int c = __popc(planes_occ(q.w) & T);
		if(c > most || (c == most && planes_less(q.w, best.w))){ best = q; most = c; }
	}
	return best;
}

// The occupied stretch lo .. hi of T in the word w; false: nothing there, a hole inside, or a slot with more than one base.
// (No word Sequence::pack makes has a hole inside -- Word::push_back writes the next base over an EOS, word.cpp:32-41 -- so the
// hole half of the test is never true on a DB of this library: it is the definition's, which reads words, and costs one mask.)
__device__ __forceinline__ bool site_stretch(const Planes &w, uint32_t T, int &lo, int &hi)
{
	const uint32_t occ = planes_occ(w) & T;
	lo = hi = 0;
	if(!occ) return false;
	lo = (int)__builtin_ctz(occ); hi = 31 - (int)__builtin_clz(occ);
	const uint32_t span = ((hi >= 31) ? 0xFFFFFFFFu : ((1u << (hi + 1)) - 1u)) & ~((1u << lo) - 1u);
	const uint32_t multi = (w.a & (w.c | w.g | w.t)) | (w.c & (w.g | w.t)) | (w.g & w.t);
	return ((multi | ~occ) & span) == 0;
}

__device__ __forceinline__ uint32_t site_slot(uint32_t g, uint32_t cap, const uint32_t *__restrict__ touched) { return touched[g/cap]*cap + g % cap; }

// expansions of item k's oligo
__global__ __launch_bounds__(POOL_THREADS) void k_site_jobs(const uint2 *__restrict__ items, uint32_t n_items, const SiteOligoX *__restrict__ ox,
	uint32_t *__restrict__ count)
{
	const uint32_t k = blockIdx.x*blockDim.x + threadIdx.x;
	if(k < n_items) count[k] = ox[items[k].y].n_exp;
}

// rank of a slot in the odometer of Word::begin() / next() (word.h:525-647): slot 15 turns fastest, then 14 .. 0, then 31 .. 16
__device__ __forceinline__ unsigned site_rank(unsigned k) { return (k < 16u) ? 15u - k : 47u - k; }

// One duplex: expansion `expansion` of oligo o against the template the planes tw spell inside T.  Wave-uniform arguments; the
// result (tm, dH, dS, status) is lane 0's.  false: the site cannot be spelled, no DP ran and no wave_sync was passed.
// (pcr_site_variants melts a variant's planes & T through this: every slot read lies in T.)
__device__ __forceinline__ bool site_melt(thermo::Engine<1> &e, thermo::WaveSlab &w, unsigned lane, const PoolOligo &o, float log_strand,
	const Planes &tw, uint32_t T, unsigned expansion, float4 &out)
{
	using namespace thermo;
	int lo, hi;
	if(!site_stretch(tw, T, lo, hi)){                                              // no DP for a site that cannot be spelled
		out = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(SITE_ST_NO_TM));
		return false;
	}
	const int qlen = o.stop - o.start + 1, tlen = hi - lo + 1;                     // 1 .. 32 both (the host refuses oligos with holes)
	e.log_strand = log_strand; e.qlen = qlen; e.tlen = tlen;
	if(lane <= MAXL){
		const int i = (int)lane;
		unsigned char qc = (unsigned char)bE, tc = (unsigned char)bE;             // "one past the end" is the non-pairing code E
		auto base_set = [&](unsigned s) -> unsigned { return ((o.m.a >> s) & 1u) | (((o.m.c >> s) & 1u) << 1) | (((o.m.g >> s) & 1u) << 2) | (((o.m.t >> s) & 1u) << 3); };
		if(i < qlen){
			// expansion index -> this slot's digit: mixed radix over the degenerate slots in the odometer's order, lowest base first
			const unsigned s = (unsigned)(o.start + i), rk = site_rank(s);
			unsigned div = 1;
			for(unsigned p = 0;p < 32u;++p){
				const unsigned d = (unsigned)__popc(base_set(p));
				if(d > 1u && site_rank(p) < rk) div *= d;
			}
			unsigned set = base_set(s);
			const unsigned d = max((unsigned)__popc(set), 1u);
			for(unsigned skip = (expansion/div) % d;skip;--skip) set &= set - 1u;
			qc = (unsigned char)(set ? (unsigned)__ffs(set) - 1u : 0u);
		}
		if(i < tlen){
			// the complement of the template bases, highest slot first
			const unsigned s = (unsigned)(hi - i);
			const unsigned b = ((tw.c >> s) & 1u) | (((tw.g >> s) & 1u) << 1) | (((tw.t >> s) & 1u)*3u);
			tc = (unsigned char)(3u - b);
		}
		w.q[i] = qc; w.t[i] = tc;
	}
	wave_sync();
	const int mxs = e.fill_wave(e.q, e.qlen, e.t, e.qlen, e.tlen, 0);
	wave_sync();
	collect_rows(e, e.qlen, e.tlen, 0, mxs, w.rowmask);
	wave_sync();
	unsigned status = 0;
	const float tm = enumerate_parallel<false>(e, w.par, w.rowmask, e.qlen, false, status);
	if(lane == 0){
		// enumerate_parallel reports the winner's Tm only; its energies are still in the lanes' slabs: the same merge again
		// (lowest dG, earliest cell on a tie).  This is a copy of the rule at the end of enumerate_parallel (pcr_thermo.inc):
		// the two must change together.
		int win = -1;
		float wdg = 0.0f, dH = 0.0f, dS = 0.0f;
		for(int l = 0;l < WAVE_PAR;++l){
			const ParLane &L = w.par[l];
			if(L.win < 0) continue;
			const float dgl = L.best.dH - TARGET_T*L.best.dS;
			if(win < 0 || dgl < wdg || (dgl == wdg && L.win < win)){ win = L.win; wdg = dgl; dH = L.best.dH; dS = L.best.dS; }
		}
		out = make_float4(tm, dH, dS, __uint_as_float((status & 1u) ? SITE_ST_ERROR : 0u));
	}
	wave_sync();                                                                   // before the next job overwrites the sequences
	return true;
}

// One LDS copy of the dG table and this wave's slab behind it: the engine every melting kernel of this file sets up.
__device__ __forceinline__ thermo::WaveSlab &site_engine(int *lds, const int *__restrict__ dg_global, float log_na, unsigned wave, thermo::Engine<1> &e)
{
	using namespace thermo;
	WaveSlab &w = ((WaveSlab *)(lds + 49*49))[wave];
	for(int i = threadIdx.x;i < 49*49;i += SITE_THREADS) lds[i] = dg_global[i];
	__syncthreads();                                                               // the only workgroup barrier
	e.dg = lds; e.log_na = log_na;
	e.q = w.q; e.t = w.t;
	e.mx.M = w.si;
	e.mx.tr = w.ss;
	return w;
}

// Job j = expansion j - joff[k] of item k, joff[k] <= j < joff[k + 1]: (tm, dH, dS, status) -> res[j].
__global__ __launch_bounds__(SITE_THREADS) void k_site_tm(const DevEntry *__restrict__ db, uint32_t cap, const uint32_t *__restrict__ touched,
	const uint32_t *__restrict__ seg_hi, const uint2 *__restrict__ items, uint32_t n_items, const uint64_t *__restrict__ joff, uint32_t n_jobs,
	const PoolOligo *__restrict__ oligos, const SiteOligoX *__restrict__ ox, const int *__restrict__ dg_global, float log_na, float4 *__restrict__ res)
{
	using namespace thermo;
	extern __shared__ int site_lds[];                                             // dg [49*49] | SITE_WAVES slabs
	const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63u;
	Engine<1> e;
	WaveSlab &w = site_engine(site_lds, dg_global, log_na, wave, e);
	for(unsigned j = blockIdx.x*SITE_WAVES + wave;j < n_jobs;j += gridDim.x*SITE_WAVES){   // uniform per wave
		unsigned k = 0, above = n_items;                                           // joff[k] <= j < joff[above]
		while(above - k > 1u){
			const unsigned mid = k + (above - k)/2u;
			if(joff[mid] <= (uint64_t)j) k = mid; else above = mid;
		}
		const uint2 it = items[k];
		const PoolOligo o = oligos[it.y];
		const uint32_t slot = site_slot(it.x, cap, touched);
		const uint32_t T = site_window(o.start, o.stop);
		const DevEntry en = site_pick(db, slot, seg_hi[db[slot].seq], o, T);
		float4 v;
		site_melt(e, w, lane, o, ox[it.y].log_strand, en.w, T, j - (unsigned)joff[k], v);
		if(lane == 0) res[j] = v;
	}
}

struct alignas(8) ItemTm { float tm; uint32_t no_tm; };                        // tm_max of the item's site (0 with NO_TM) and its NO_TM bit: one 8-byte load

// Item k: its expansions joff[k] .. joff[k + 1] - 1 in index order; the highest Tm (k_site_reduce's rule for tm_max: strict >,
// the lowest index wins, no float atomics).  Indexed by item: the join kernels read a product's two Tm as two array reads.
__global__ __launch_bounds__(POOL_THREADS) void k_item_tm(const uint64_t *__restrict__ joff, uint32_t n_items, const float4 *__restrict__ res,
	ItemTm *__restrict__ item_tm, uint32_t *__restrict__ error)
{
	const uint32_t k = blockIdx.x*blockDim.x + threadIdx.x;
	if(k >= n_items) return;
	const uint64_t j0 = joff[k], j1 = joff[k + 1];
	float tm = 0.0f;
	uint32_t st = 0;
	for(uint64_t j = j0;j < j1;++j){
		const float4 v = res[j];
		st |= __float_as_uint(v.w);
		if(j == j0 || v.x > tm) tm = v.x;
	}
	ItemTm r;
	r.no_tm = (st & SITE_ST_NO_TM) ? 1u : 0u;
	r.tm = r.no_tm ? 0.0f : tm;
	if(st & SITE_ST_ERROR) atomicOr(error, 1u);
	item_tm[k] = r;
}

// The melt stage over the ni items of B.items: k_site_jobs + a scan -> B.joff; k_site_tm, one wave per (item, expansion) ->
// B.res[job]; and with B.item_tm, k_item_tm -> item_tm[] (kept as uint2 by the handle: the struct is this file's) after zeroing
// its error flag B.flag[0], which one call leaves for the next.  B.cnt holds ni + 1 elements.  The jobs are queued, not waited for.
int melt_items(const std::string &who, pcr_ctx *ctx, const SeqSet &S, const PoolOligo *d_ol, const SiteOligoX *d_olx, uint32_t ni, float salt,
	const ItemBufs &B)
{
	static_assert(sizeof(ItemTm) == sizeof(uint2), "table layout");
	int rc;
	const unsigned grid_i = (ni + POOL_THREADS - 1)/POOL_THREADS;
	if(B.item_tm){                                                               // (first, so that k_site_tm and k_item_tm follow each other on the stream)
		if((rc = B.flag->ensure(1)) != PCR_OK) return rc;
		HIP_TRY(hipMemsetAsync(B.flag->p, 0, sizeof(uint32_t), ctx->stream));
	}
	hipLaunchKernelGGL(k_site_jobs, dim3(grid_i), dim3(POOL_THREADS), 0, ctx->stream, (const uint2 *)B.items->p, ni, d_olx, B.cnt->p);
	HIP_TRY(hipGetLastError());
	uint64_t n_jobs64 = 0;
	if((rc = scan_total(ctx, B.cnt->p, *B.joff, *B.tmp, ni, n_jobs64)) != PCR_OK) return rc;
	if(n_jobs64 >= POOL_MAX_ITEMS){ g_err = who + ": too many (site, expansion) jobs"; return PCR_ERR_CAPACITY; }
	const uint32_t n_jobs = (uint32_t)n_jobs64;
	if((rc = ensure_dg_table(ctx, salt)) != PCR_OK) return rc;
	if(!ctx->site_attr_set){
		HIP_TRY(hipFuncSetAttribute((const void *)k_site_tm, hipFuncAttributeMaxDynamicSharedMemorySize, (int)SITE_LDS));
		ctx->site_attr_set = true;
	}
	if((rc = B.res->ensure(n_jobs)) != PCR_OK) return rc;
	// at most one block per CU (a block takes most of a CU's LDS), the waves striding over the jobs
	const unsigned grid_j = std::max(1u, std::min<unsigned>((n_jobs + SITE_WAVES - 1)/SITE_WAVES, (unsigned)ctx->n_cu));
	hipLaunchKernelGGL(k_site_tm, dim3(grid_j), dim3(SITE_THREADS), SITE_LDS, ctx->stream, S.db.p, S.db_cap, S.touched.p, S.d_seg_hi,
		(const uint2 *)B.items->p, ni, (const uint64_t *)B.joff->p, n_jobs, d_ol, d_olx, (const int *)ctx->th_dg.p, logf(salt), B.res->p);
	HIP_TRY(hipGetLastError());
	if(!B.item_tm) return PCR_OK;
	if((rc = B.item_tm->ensure(ni)) != PCR_OK) return rc;
	hipLaunchKernelGGL(k_item_tm, dim3(grid_i), dim3(POOL_THREADS), 0, ctx->stream, (const uint64_t *)B.joff->p, ni, (const float4 *)B.res->p,
		(ItemTm *)B.item_tm->p, B.flag->p);
	HIP_TRY(hipGetLastError());
	return PCR_OK;
}

// One oligo of a melting entry point -> its table entries, or false with g_err saying why it is refused.  what: "an oligo", "a
// primer", "a probe"; conc, conc_name: the oligo's strand concentration and what the message calls it.  melt = false (no
// thermodynamics asked for): no concentration is looked at.
bool site_oligo(const std::string &who, const char *what, const pcr_word128 &wd, float thr2, bool melt, float conc, const char *conc_name,
	float template_strand, PoolOligo &p, SiteOligoX &x)
{
	OligoDev d; fill_oligo(d, wd.w, thr2);
	const uint32_t occ = pcrhost::planes_occupied(d.m);
	if(!occ || __builtin_popcount(occ) != d.stop - d.start + 1){
		g_err = who + ": " + what + " is empty or has a hole between its ends (NucCruc::set_query throws)"; return false;
	}
	const double degen = pcrhost::planes_degeneracy(d.m);
	if(degen > (double)PCR_SITE_MAX_EXPANSIONS){ g_err = who + ": " + what + " has more than PCR_SITE_MAX_EXPANSIONS expansions"; return false; }
	p.m = d.m; p.floor2 = d.floor2; p.start = d.start; p.stop = d.stop; p.pad = 0;
	x.n_exp = (uint32_t)degen; x.log_strand = 0.0f;
	if(melt){
		const float ca = (float)(conc/degen), cb = template_strand;
		const float strand = (ca > cb) ? ca - 0.5f*cb : cb - 0.5f*ca;              // nuc_cruc.h:832-837
		if(!(strand > 0.0f)){
			g_err = who + ": the strand concentration of " + what + "'s duplex is zero (" + conc_name + " / degeneracy and template_strand both 0)"; return false;
		}
		x.log_strand = logf(strand);
	}
	return true;
}

// The distinct oligos of a panel or pool, in order of first appearance (as pcr_pool_products), appended to ol / olx and numbered by
// their place in ol; oligo_id[s] of every oligo listed before a refusal is written.  args = NULL: no thermodynamics (site_oligo's melt = false).
int site_oligo_table(const std::string &who, const char *what, const char *conc_name, const pcr_pair *pairs, uint32_t n_pairs, float threshold,
	const pcr_thermo_args *args, float template_strand, uint32_t *oligo_id, std::vector<PoolOligo> &ol, std::vector<SiteOligoX> &olx)
{
	std::map<std::pair<uint64_t, uint64_t>, uint32_t> id_of;
	const float thr2 = threshold*threshold;                                      // pcr_assay.cpp:775-776
	for(uint32_t s = 0;s < 2*n_pairs;++s){
		const pcr_word128 &wd = (s & 1) ? pairs[s/2].r : pairs[s/2].f;
		auto ins = id_of.insert(std::make_pair(std::make_pair(wd.w[0], wd.w[1]), (uint32_t)ol.size()));
		if(ins.second){
			PoolOligo p; SiteOligoX x;
			if(!site_oligo(who, what, wd, thr2, args != nullptr, args ? args->primer_strand : 0.0f, conc_name, template_strand, p, x)) return PCR_ERR_ARG;
			ol.push_back(p); olx.push_back(x);
		}
		oligo_id[s] = ins.first->second;
	}
	return PCR_OK;
}

// sort keys of the items: (loc5, strand) first, then stably (oligo, sequence)
__global__ __launch_bounds__(POOL_THREADS) void k_site_key1(const DevEntry *__restrict__ db, uint32_t cap, const uint32_t *__restrict__ touched,
	const uint2 *__restrict__ items, uint32_t n_items, const PoolOligo *__restrict__ oligos, uint64_t *__restrict__ key, uint32_t *__restrict__ ord)
{
	const uint32_t k = blockIdx.x*blockDim.x + threadIdx.x;
	if(k >= n_items) return;
	const uint2 it = items[k];
	const DevEntry e = db[site_slot(it.x, cap, touched)];
	const PoolOligo o = oligos[it.y];
	const int32_t loc5 = (e.strand == 1) ? e.loc + o.start : e.loc - o.stop;      // sequence.h:57-65
	key[k] = ((uint64_t)((uint32_t)loc5 ^ 0x80000000u) << 1) | (e.strand - 1u);   // signed order
	ord[k] = k;
}

__global__ __launch_bounds__(POOL_THREADS) void k_site_key2(const DevEntry *__restrict__ db, uint32_t cap, const uint32_t *__restrict__ touched,
	const uint2 *__restrict__ items, const uint32_t *__restrict__ ord, uint32_t n_items, uint32_t seq_bits, uint64_t *__restrict__ key)
{
	const uint32_t r = blockIdx.x*blockDim.x + threadIdx.x;
	if(r >= n_items) return;
	const uint2 it = items[ord[r]];
	key[r] = ((uint64_t)it.y << seq_bits) | db[site_slot(it.x, cap, touched)].seq;
}

// Record r = item ord[r]: its expansions in index order; the highest Tm (the lowest index on a tie) gives dH and dS.
__global__ __launch_bounds__(POOL_THREADS) void k_site_reduce(const DevEntry *__restrict__ db, uint32_t cap, const uint32_t *__restrict__ touched,
	const uint32_t *__restrict__ seg_hi, const uint2 *__restrict__ items, const uint32_t *__restrict__ ord, uint32_t n_items,
	const uint64_t *__restrict__ joff, const PoolOligo *__restrict__ oligos, const float4 *__restrict__ res, pcr_site *__restrict__ out,
	uint32_t *__restrict__ error)
{
	const uint32_t r = blockIdx.x*blockDim.x + threadIdx.x;
	if(r >= n_items) return;
	const uint32_t k = ord[r];
	const uint2 it = items[k];
	const PoolOligo o = oligos[it.y];
	const uint32_t slot = site_slot(it.x, cap, touched);
	const DevEntry en = site_pick(db, slot, seg_hi[db[slot].seq], o, site_window(o.start, o.stop));
	pcr_site s;
	s.oligo = it.y; s.sequence = en.seq; s.strand = en.strand;
	s.loc5 = (en.strand == 1) ? en.loc + o.start : en.loc - o.stop;              // sequence.h:57-75
	s.loc3 = (en.strand == 1) ? en.loc + o.stop : en.loc - o.start;
	s.matches = (uint32_t)__popc((en.w.a & o.m.a) | (en.w.c & o.m.c) | (en.w.g & o.m.g) | (en.w.t & o.m.t));
	const uint64_t j0 = joff[k], j1 = joff[k + 1];
	s.n_expansions = (uint32_t)(j1 - j0); s.flags = 0;
	s.tm_max = s.tm_min = s.dH = s.dS = 0.0f;
	uint32_t st = 0;
	for(uint64_t j = j0;j < j1;++j){
		const float4 v = res[j];
		st |= __float_as_uint(v.w);
		if(j == j0 || v.x > s.tm_max){ s.tm_max = v.x; s.dH = v.y; s.dS = v.z; }
		if(j == j0 || v.x < s.tm_min) s.tm_min = v.x;
	}
	if(st & SITE_ST_NO_TM){ s.flags = PCR_SITE_NO_TM; s.tm_max = s.tm_min = s.dH = s.dS = 0.0f; }
	if(st & SITE_ST_ERROR) atomicOr(error, 1u);
	out[r] = s;
}

} // namespace

extern "C" {

int64_t pcr_site_tm(pcr_ctx *ctx, pcr_set which, const pcr_pair *pairs, uint32_t n_pairs, float threshold,
	const pcr_thermo_args *args, float template_strand, uint32_t *oligo_id, pcr_site *out, uint64_t cap)
{
	static_assert(sizeof(pcr_site) == 48, "record layout");
	static_assert(PCR_SITE_MAX_EXPANSIONS <= 256, "a job's digit arithmetic is 32-bit");
	// ---- the arguments, before the handle
	if(!set_ok(which)){ g_err = "pcr_site_tm: unknown sequence set"; return PCR_ERR_ARG; }
	if(which != PCR_SET_TARGET && which != PCR_SET_BACKGROUND){ g_err = "pcr_site_tm: PCR_SET_MULTIPLEX is not supported (PCR_SET_TARGET or PCR_SET_BACKGROUND)"; return PCR_ERR_ARG; }
	if(!args || (n_pairs && (!pairs || !oligo_id)) || (cap && !out)){ g_err = "pcr_site_tm: bad argument"; return PCR_ERR_ARG; }
	if(n_pairs > PCR_POOL_MAX_PAIRS){ g_err = "pcr_site_tm: panel larger than PCR_POOL_MAX_PAIRS"; return PCR_ERR_ARG; }
	if(!(template_strand >= 0.0f) || !(args->primer_strand >= 0.0f)){ g_err = "pcr_site_tm: negative strand concentration (NucCruc::strand, nuc_cruc.h:818-826)"; return PCR_ERR_ARG; }
	if(!(args->salt >= 1.0e-6f && args->salt <= 1.0f)){ g_err = "pcr_site_tm: salt outside [1e-6, 1] (NucCruc::salt, nuc_cruc.h:780-788)"; return PCR_ERR_ARG; }
	std::vector<PoolOligo> ol;
	std::vector<SiteOligoX> olx;
	if(site_oligo_table("pcr_site_tm", "an oligo", "primer_strand", pairs, n_pairs, threshold, args, template_strand, oligo_id, ol, olx) != PCR_OK) return PCR_ERR_ARG;
	if(!ctx){ g_err = "pcr_site_tm: null handle"; return PCR_ERR_ARG; }
	{ const int drc = drain(ctx); if(drc != PCR_OK) return drc; }
	HIP_TRY(hipSetDevice(ctx->device));
	SeqSet &S = ctx->sets[which];
	if(!S.have_db){ g_err = "pcr_site_tm: no word DB (call pcr_select_words or pcr_select_sites first)"; return PCR_ERR_STATE; }
	if(n_pairs == 0) return 0;
	{ const int erc = ensure_touched(ctx, S); if(erc != PCR_OK) return erc; }
	if(S.n_entries == 0 || S.n_touched == 0) return 0;
	const uint32_t n_ol = (uint32_t)ol.size();
	int rc;
	const size_t ol_bytes = ol.size()*sizeof(PoolOligo), olx_bytes = olx.size()*sizeof(SiteOligoX);
	if((rc = ctx->site_in.ensure(ol_bytes + olx_bytes)) != PCR_OK) return rc;
	const PoolOligo *d_ol = (const PoolOligo *)ctx->site_in.p;
	const SiteOligoX *d_olx = (const SiteOligoX *)(ctx->site_in.p + ol_bytes);
	HIP_TRY(hipMemcpyAsync(ctx->site_in.p, ol.data(), ol_bytes, hipMemcpyHostToDevice, ctx->stream));
	HIP_TRY(hipMemcpyAsync(ctx->site_in.p + ol_bytes, olx.data(), olx_bytes, hipMemcpyHostToDevice, ctx->stream));
	// ---- 1. the items; 2. job offsets; 3. the jobs
	const ItemBufs B{&ctx->site_tmp, &ctx->site_cnt, &ctx->site_eoff, &ctx->site_items, &ctx->site_joff, &ctx->site_res};   // (k_site_reduce, not k_item_tm, reads the jobs)
	uint64_t n_items = 0;
	if((rc = item_count(ctx, S, d_ol, n_ol, B, n_items)) != PCR_OK) return rc;
	if(n_items >= POOL_MAX_ITEMS){ g_err = "pcr_site_tm: too many sites"; return PCR_ERR_CAPACITY; }
	if(n_items == 0 || n_items > cap) return (int64_t)n_items;                   // count only: out is left as it is
	if((rc = item_fill(ctx, S, d_ol, n_ol, B, n_items)) != PCR_OK) return rc;
	const uint32_t ni = (uint32_t)n_items;
	const unsigned grid_i = (ni + POOL_THREADS - 1)/POOL_THREADS;
	if((rc = ctx->site_cnt.ensure((size_t)ni + 1)) != PCR_OK) return rc;        // (the entry counts are spent)
	if((rc = melt_items("pcr_site_tm", ctx, S, d_ol, d_olx, ni, args->salt, B)) != PCR_OK) return rc;
	if((rc = ctx->site_flag.ensure(1)) != PCR_OK) return rc;
	HIP_TRY(hipMemsetAsync(ctx->site_flag.p, 0, sizeof(uint32_t), ctx->stream));
	// ---- 4. the record order, the records
	if((rc = ctx->site_keys.ensure(2*(size_t)ni)) != PCR_OK) return rc;
	if((rc = ctx->site_ord.ensure(2*(size_t)ni)) != PCR_OK) return rc;
	if((rc = ctx->site_rec.ensure(ni)) != PCR_OK) return rc;
	uint64_t *k0 = ctx->site_keys.p, *k1 = k0 + ni;
	uint32_t *o0 = ctx->site_ord.p, *o1 = o0 + ni;
	hipLaunchKernelGGL(k_site_key1, dim3(grid_i), dim3(POOL_THREADS), 0, ctx->stream, S.db.p, S.db_cap, S.touched.p, (const uint2 *)ctx->site_items.p, ni, d_ol, k0, o0);
	HIP_TRY(hipGetLastError());
	const unsigned seq_bits = pool_bits(S.n), oligo_bits = pool_bits(n_ol);
	size_t t1 = 0, t2 = 0;
	HIP_TRY(rocprim::radix_sort_pairs(nullptr, t1, k0, k1, o0, o1, ni, 0, 33, ctx->stream));
	HIP_TRY(rocprim::radix_sort_pairs(nullptr, t2, k0, k1, o1, o0, ni, 0, oligo_bits + seq_bits, ctx->stream));
	if((rc = ctx->site_tmp.ensure(std::max(t1, t2) + 16)) != PCR_OK) return rc;
	HIP_TRY(rocprim::radix_sort_pairs(ctx->site_tmp.p, t1, k0, k1, o0, o1, ni, 0, 33, ctx->stream));
	hipLaunchKernelGGL(k_site_key2, dim3(grid_i), dim3(POOL_THREADS), 0, ctx->stream, S.db.p, S.db_cap, S.touched.p, (const uint2 *)ctx->site_items.p, (const uint32_t *)o1, ni, seq_bits, k0);
	HIP_TRY(hipGetLastError());
	HIP_TRY(rocprim::radix_sort_pairs(ctx->site_tmp.p, t2, k0, k1, o1, o0, ni, 0, oligo_bits + seq_bits, ctx->stream));   // (stable)
	hipLaunchKernelGGL(k_site_reduce, dim3(grid_i), dim3(POOL_THREADS), 0, ctx->stream, S.db.p, S.db_cap, S.touched.p, S.d_seg_hi,
		(const uint2 *)ctx->site_items.p, (const uint32_t *)o0, ni, (const uint64_t *)ctx->site_joff.p, d_ol, (const float4 *)ctx->site_res.p, ctx->site_rec.p, ctx->site_flag.p);
	HIP_TRY(hipGetLastError());
	uint32_t bad = 0;
	HIP_TRY(hipMemcpyAsync(out, ctx->site_rec.p, (size_t)ni*sizeof(pcr_site), hipMemcpyDeviceToHost, ctx->stream));
	HIP_TRY(hipMemcpyAsync(&bad, ctx->site_flag.p, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
	HIP_TRY(hipStreamSynchronize(ctx->stream));
	if(bad & 1u){ g_err = "pcr_site_tm: internal trace-back error"; return PCR_ERR_RANGE; }
	return (int64_t)n_items;
}

} // extern "C"
