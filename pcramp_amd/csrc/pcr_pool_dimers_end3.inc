// Which oligos of a pool extend on each other (pcr_pool_dimers_end3; included by pcr_device.hip after pcr_pool_dimers.inc, whose
// plan, tables, pdim_code, pdim_floor_near and pdim_winner it shares).
//
// A placement j of a duplex (expansion of the query x, expansion of the target y) puts x's 3' base opposite y[j]; it qualifies
// if the Watson-Crick run from that base on has min_run pairs and j >= min_extension -- the definition is written out at
// pcr_pool_dimers_end3 in include/pcramp_hip.h.  Nothing is spelt on the host:
//   1. k_dimer_end3_scan, a lane per placement (32 lanes per duplex, two duplexes per wave): the 32 lanes spell one base of x
//      and of y each (pdim_code), four ballots per strand turn them into A / C / G / T bit planes, and placement j is bit
//      arithmetic on them: reverse x, shift y by j, AND the complementary planes.  run = the trailing ones, overlap_matches =
//      the popcount.  It runs twice: <false> counts the qualifying placements per duplex, an exclusive scan gives each duplex
//      its place, <true> writes the jobs there (a lane's rank among its duplex's qualifying lanes: a ballot, no atomic).  The
//      job list is in record order: cell, duplex, j.
//   2. k_dimer_end3_melt: one wave per job, k_pool_dimer's shape (THERMO_WAVES waves around one LDS copy of the dG table, at
//      most one block per CU, grid-strided).  The lanes spell the run's two strings into the slab and the engine's hetero path
//      runs on them.  At most POOL_DIMER_END3_BATCH_JOBS jobs per launch.
//   3. k_dimer_end3_merge, a thread per cell, walks the part of the cell's jobs a launch melted, in order (lowest dG, the longer
//      run on a tie, else the earlier: no float atomics) and carries the best in the cell's record from launch to launch.
//      Keep flags, an exclusive scan and a compacting kernel put the kept placements of a launch, and the kept cells of a
//      batch, into record order.
// Cells go in batches of consecutive whole cells of at most POOL_DIMER_END3_BATCH_DUPLEXES duplexes (DESIGN.md has the bounds).
// The call owns its scratch (pcr_ctx::pde3_*, and pdim_in / pdim_tmp / pdim_flag, which every call fills anew); the dG table
// is the handle's (th_dg, keyed by its salt).
// The batch loop is end3_batches, which pcr_pool_conflicts_ext runs too, with a dense device array in place of the caller's
// host arrays (End3Out): then a batch's records are merged where they stay and nothing is compacted or downloaded.

namespace {

constexpr uint32_t POOL_DIMER_END3_BATCH_DUPLEXES = 1u << 20;                   // mirrored in api.py; 8 MB of counts and offsets
constexpr uint32_t POOL_DIMER_END3_BATCH_JOBS = 1u << 17;                       // mirrored in api.py; 2 MB of float4 per launch
static_assert(POOL_DIMER_END3_BATCH_DUPLEXES >= 65536u, "a batch holds the largest cell");
static_assert(POOL_DIMER_END3_BATCH_DUPLEXES <= (1u << 20), "End3Job keeps a batch's cell number in 20 bits");

// One job: x = cell in the batch (20 bits) | j << 20 (5 bits) | (run - 1) << 25 (5 bits); y = duplex in the cell (16 bits) | overlap_matches << 16
__host__ __device__ inline uint2 end3_job(uint32_t cell, uint32_t j, uint32_t run, uint32_t dup, uint32_t matches)
{
	return make_uint2(cell | (j << 20) | ((run - 1u) << 25), dup | (matches << 16));
}
struct End3Job { uint32_t cell, j, run, dup, matches; };
__device__ __forceinline__ End3Job end3_unpack(uint2 v)
{
	End3Job b;
	b.cell = v.x & 0xFFFFFu; b.j = (v.x >> 20) & 31u; b.run = ((v.x >> 25) & 31u) + 1u; b.dup = v.y & 0xFFFFu; b.matches = v.y >> 16;
	return b;
}

// Duplex d of the whole matrix -> its cell (q, t) and expansions (k_pool_dimer's two guided searches; on the diagonal iq = it).
__device__ __forceinline__ void end3_locate(const DimerPlan &P, unsigned d, unsigned &q, unsigned &t, unsigned &iq, unsigned &it)
{
	const unsigned n_exp_all = P.pref[P.n];
	q = pdim_floor_near(P.row, P.n, d, (unsigned)((float)d*(float)P.n/(float)P.row[P.n]));
	const unsigned dq = P.ol[q].n_exp, r = d - P.row[q], diag0 = dq*P.pref[q];
	t = q; iq = it = r - diag0;
	if(r >= diag0 && r < diag0 + dq) return;
	const unsigned rr = (r < diag0) ? r : r - dq + dq*dq;                         // as if the diagonal cell were D(q)^2 wide
	t = pdim_floor_near(P.pref, P.n, rr/dq, ((rr/dq)*P.n)/n_exp_all);
	const unsigned rem = rr - dq*P.pref[t], dt = P.ol[t].n_exp;
	iq = rem/dt; it = rem % dt;
}

// Duplex d0 + dl, dl < nd, placement j = the lane within its half wave.  FILL false: cnt[dl] = the qualifying placements.
// FILL true: their jobs at off[dl] .., j ascending.
template<bool FILL> __global__ __launch_bounds__(POOL_THREADS) void k_dimer_end3_scan(DimerPlan P, uint32_t c0, uint32_t d0, uint32_t nd,
	uint32_t min_run, uint32_t min_extension, uint32_t *__restrict__ cnt, const uint32_t *__restrict__ off, uint2 *__restrict__ jobs)
{
	const uint32_t g = blockIdx.x*blockDim.x + threadIdx.x;
	const bool valid = (g >> 5) < nd;                                             // (no early return: the ballots are the whole wave's)
	const uint32_t dl = valid ? (g >> 5) : nd - 1u, j = g & 31u, shift = threadIdx.x & 32u;
	unsigned q, t, iq, it;
	end3_locate(P, d0 + dl, q, t, iq, it);
	const DimerOligo oq = P.ol[q], ot = P.ol[t];
	const uint32_t Lx = (uint32_t)(oq.stop - oq.start + 1), Ly = (uint32_t)(ot.stop - ot.start + 1);
	const unsigned cx = (j < Lx) ? pdim_code(oq.m, (unsigned)oq.start + j, iq, oq.n_exp) : 4u;   // lane j spells base j of both strands
	const unsigned cy = (j < Ly) ? pdim_code(ot.m, (unsigned)ot.start + j, it, ot.n_exp) : 4u;
	uint32_t X[4], Y[4];
	for(unsigned b = 0;b < 4u;++b){
		X[b] = __brev((uint32_t)(__ballot(cx == b) >> shift)) >> (32u - Lx);       // x reversed: bit k is x[Lx - 1 - k]
		Y[b] = (uint32_t)(__ballot(cy == b) >> shift);
	}
	const uint32_t overlap = (j < Ly) ? min(Lx, Ly - j) : 0u;
	const uint32_t mask = (overlap >= 32u) ? ~0u : (1u << overlap) - 1u;
	const uint32_t wc = ((X[0] & (Y[3] >> j)) | (X[3] & (Y[0] >> j)) | (X[1] & (Y[2] >> j)) | (X[2] & (Y[1] >> j))) & mask;   // codes: A 0, C 1, G 2, T 3
	const uint32_t run = (wc == ~0u) ? 32u : (uint32_t)__ffs((int)~wc) - 1u;
	const bool qual = valid && run >= min_run && j >= min_extension && overlap > 0u;
	const uint32_t qb = (uint32_t)(__ballot(qual) >> shift);
	if(!FILL){
		if(valid && j == 0u) cnt[dl] = (uint32_t)__popc(qb);
	}
	else if(qual){
		const uint32_t cell = q*P.n + t - c0, dup = (q == t) ? iq : iq*ot.n_exp + it;
		jobs[off[dl] + (uint32_t)__popc(qb & ((1u << j) - 1u))] = end3_job(cell, j, run, dup, (uint32_t)__popc(wc));
	}
}

// Cell c0 + k, k < n_cells: its record before any placement is melted; off = the exclusive scan of the batch's counts.
__global__ __launch_bounds__(POOL_THREADS) void k_dimer_end3_cells(DimerPlan P, uint32_t c0, uint32_t n_cells, uint32_t d0, const uint32_t *__restrict__ off,
	pcr_pool_dimer_end3 *__restrict__ rec)
{
	const uint32_t k = blockIdx.x*blockDim.x + threadIdx.x;
	if(k >= n_cells) return;
	const uint32_t c = c0 + k, q = c/P.n, t = c % P.n;
	const uint32_t dq = P.ol[q].n_exp, dt = P.ol[t].n_exp;
	const uint32_t ndc = (q == t) ? dq : dq*dt, first = pdim_before(P.row, P.pref, q, t, dq) - d0;
	pcr_pool_dimer_end3 d;
	d.query_oligo = q; d.target_oligo = t; d.n_duplexes = ndc; d.n_placements = off[first + ndc] - off[first];
	d.q_expansion = d.t_expansion = 0u;
	d.run = d.extension = d.overlap = d.overlap_matches = 0;
	d.flags = (q == t) ? PCR_DIMER_HOMO : 0u;
	d.dG = d.tm = d.dH = d.dS = 0.0f;
	rec[k] = d;
}

// Job jl < n_jobs of a launch (jobs points at its first): the run's heterodimer (tm, dH, dS, status) -> res[jl].
__global__ __launch_bounds__(PDIM_THREADS) void k_dimer_end3_melt(DimerPlan P, uint32_t c0, const uint2 *__restrict__ jobs, uint32_t n_jobs,
	const int *__restrict__ dg_global, float log_na, float4 *__restrict__ res)
{
	using namespace thermo;
	extern __shared__ int pde3_lds[];                                             // dg [49*49] | PDIM_WAVES slabs
	int *const dg = pde3_lds;
	const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63u;
	WaveSlab &w = ((WaveSlab *)(pde3_lds + 49*49))[wave];
	for(int i = threadIdx.x;i < 49*49;i += PDIM_THREADS) dg[i] = dg_global[i];
	__syncthreads();                                                               // the only workgroup barrier
	Engine<1> e;
	e.dg = dg; e.log_na = log_na;
	e.q = w.q; e.t = w.t;
	e.mx.M = w.si;
	e.mx.tr = w.ss;
	for(unsigned jl = blockIdx.x*PDIM_WAVES + wave;jl < n_jobs;jl += gridDim.x*PDIM_WAVES){   // uniform per wave
		const End3Job jb = end3_unpack(jobs[jl]);
		const unsigned c = c0 + jb.cell, q = c/P.n, t = c % P.n;
		const DimerOligo oq = P.ol[q], ot = P.ol[t];
		const unsigned iq = (q == t) ? jb.dup : jb.dup/ot.n_exp, it = (q == t) ? jb.dup : jb.dup % ot.n_exp;
		const int run = (int)jb.run;                                                // 3 .. 32, within both oligos (the scan's overlap)
		e.log_strand = P.log_off[oq.cls*P.n_cls + ot.cls];                          // the off-diagonal rule, on the diagonal too
		e.qlen = run; e.tlen = run;
		if(lane <= MAXL){
			const int i = (int)lane;
			unsigned char qc = (unsigned char)bE, tc = (unsigned char)bE;           // "one past the end" is the non-pairing code E
			if(i < run){
				qc = pdim_code(oq.m, (unsigned)(oq.stop - run + 1 + i), iq, oq.n_exp);   // x's last `run` bases
				tc = pdim_code(ot.m, (unsigned)(ot.start + (int)jb.j + i), it, ot.n_exp);   // y[j .. j + run - 1]
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
			float dH, dS;
			pdim_winner(w.par, dH, dS);
			res[jl] = make_float4(tm, dH, dS, __uint_as_float((status & 1u) ? PDIM_ST_ERROR : 0u));
		}
		wave_sync();                                                               // before the next job overwrites the sequences
	}
}

// the fields of a job that a record spells out
__device__ __forceinline__ void end3_geometry(const DimerPlan &P, uint32_t q, uint32_t t, const End3Job &jb, uint32_t &qe, uint32_t &te, uint32_t &overlap, uint32_t &flags)
{
	const DimerOligo &oq = P.ol[q], &ot = P.ol[t];
	const uint32_t Lx = (uint32_t)(oq.stop - oq.start + 1), Ly = (uint32_t)(ot.stop - ot.start + 1);
	qe = (q == t) ? jb.dup : jb.dup/ot.n_exp; te = (q == t) ? jb.dup : jb.dup % ot.n_exp;
	overlap = min(Lx, Ly - jb.j);
	flags = ((q == t) ? PCR_DIMER_HOMO : 0u) | ((jb.j + jb.run == Ly) ? PCR_DIMER_END3_MUTUAL : 0u);
}

// Cell c0 + k: the jobs of the batch numbered a .. a + n_jobs - 1 that are the cell's, in order, merged into its record (the best
// of the launches before is in it where the cell began before a).
__global__ __launch_bounds__(POOL_THREADS) void k_dimer_end3_merge(DimerPlan P, uint32_t c0, uint32_t n_cells, uint32_t d0, const uint32_t *__restrict__ off,
	const uint2 *__restrict__ jobs, uint32_t a, uint32_t n_jobs, const float4 *__restrict__ res, pcr_pool_dimer_end3 *__restrict__ rec, uint32_t *__restrict__ error)
{
	const uint32_t k = blockIdx.x*blockDim.x + threadIdx.x;
	if(k >= n_cells) return;
	const uint32_t c = c0 + k, q = c/P.n, t = c % P.n;
	const uint32_t dq = P.ol[q].n_exp, dt = P.ol[t].n_exp;
	const uint32_t ndc = (q == t) ? dq : dq*dt, first = pdim_before(P.row, P.pref, q, t, dq) - d0;
	const uint32_t f = off[first], l = off[first + ndc], lo = max(f, a), hi = min(l, a + n_jobs);
	if(lo >= hi) return;
	pcr_pool_dimer_end3 d = rec[k];
	bool has = f < a;
	uint32_t st = 0;
	for(uint32_t i = lo;i < hi;++i){
		const float4 v = res[i - a];
		const End3Job jb = end3_unpack(jobs[i]);
		const float dg = v.y - thermo::TARGET_T*v.z;
		st |= __float_as_uint(v.w);
		if(has && !(dg < d.dG || (dg == d.dG && jb.run > (uint32_t)d.run))) continue;   // (in order: the earlier duplex, then the lower j, stays on a full tie)
		uint32_t qe, te, overlap, flags;
		end3_geometry(P, q, t, jb, qe, te, overlap, flags);
		d.q_expansion = qe; d.t_expansion = te;
		d.run = (uint8_t)jb.run; d.extension = (uint8_t)jb.j; d.overlap = (uint8_t)overlap; d.overlap_matches = (uint8_t)jb.matches;
		d.flags = flags;
		d.dG = dg; d.tm = v.x; d.dH = v.y; d.dS = v.z;
		has = true;
	}
	if(st & PDIM_ST_ERROR) atomicOr(error, 1u);
	rec[k] = d;
}

// a cell is kept where it has a placement and its best one passes the filter (the best has the lowest dG of all)
__global__ __launch_bounds__(POOL_THREADS) void k_dimer_end3_cell_keep(const pcr_pool_dimer_end3 *__restrict__ rec, uint32_t n_cells, int keep_all, float dg_max,
	uint32_t *__restrict__ keep)
{
	const uint32_t k = blockIdx.x*blockDim.x + threadIdx.x;
	if(k < n_cells) keep[k] = (rec[k].n_placements > 0u && (keep_all || rec[k].dG <= dg_max)) ? 1u : 0u;
}

__global__ __launch_bounds__(POOL_THREADS) void k_dimer_end3_cell_compact(const pcr_pool_dimer_end3 *__restrict__ rec, const uint32_t *__restrict__ keep,
	const uint32_t *__restrict__ off, uint32_t n_cells, pcr_pool_dimer_end3 *__restrict__ out)
{
	const uint32_t k = blockIdx.x*blockDim.x + threadIdx.x;
	if(k < n_cells && keep[k]) out[off[k]] = rec[k];
}

// a launch's placements: kept where the placement's own dG passes
__global__ __launch_bounds__(POOL_THREADS) void k_dimer_end3_place_keep(const float4 *__restrict__ res, uint32_t n_jobs, float dg_max, uint32_t *__restrict__ keep)
{
	const uint32_t i = blockIdx.x*blockDim.x + threadIdx.x;
	if(i < n_jobs){ const float4 v = res[i]; keep[i] = (v.y - thermo::TARGET_T*v.z <= dg_max) ? 1u : 0u; }
}

// ... and written in job order: koff = exclusive scan of keep
__global__ __launch_bounds__(POOL_THREADS) void k_dimer_end3_place_write(DimerPlan P, uint32_t c0, const uint2 *__restrict__ jobs, const float4 *__restrict__ res,
	const uint32_t *__restrict__ keep, const uint32_t *__restrict__ koff, uint32_t n_jobs, pcr_dimer_placement *__restrict__ out)
{
	const uint32_t i = blockIdx.x*blockDim.x + threadIdx.x;
	if(i >= n_jobs || !keep[i]) return;
	const End3Job jb = end3_unpack(jobs[i]);
	const uint32_t c = c0 + jb.cell, q = c/P.n, t = c % P.n;
	const float4 v = res[i];
	uint32_t qe, te, overlap, flags;
	end3_geometry(P, q, t, jb, qe, te, overlap, flags);
	pcr_dimer_placement p;
	p.query_oligo = q; p.target_oligo = t; p.q_expansion = qe; p.t_expansion = te;
	p.run = (uint8_t)jb.run; p.extension = (uint8_t)jb.j; p.overlap = (uint8_t)overlap; p.overlap_matches = (uint8_t)jb.matches;
	p.flags = flags;
	p.dG = v.y - thermo::TARGET_T*v.z; p.tm = v.x; p.dH = v.y; p.dS = v.z;
	out[koff[i]] = p;
}

// koff[0 .. n] = exclusive scan of keep[0 .. n - 1] (both hold n + 1 words); *total = koff[n], there when the stream is synchronised
int end3_scan(pcr_ctx *ctx, uint32_t *keep, uint32_t *koff, uint32_t n, uint32_t *total)
{
	int rc;
	HIP_TRY(hipMemsetAsync(keep + n, 0, sizeof(uint32_t), ctx->stream));
	size_t tmp = 0;
	HIP_TRY(rocprim::exclusive_scan(nullptr, tmp, keep, koff, uint32_t(0), (size_t)n + 1, rocprim::plus<uint32_t>(), ctx->stream));
	if((rc = ctx->pdim_tmp.ensure(tmp + 16)) != PCR_OK) return rc;
	HIP_TRY(rocprim::exclusive_scan(ctx->pdim_tmp.p, tmp, keep, koff, uint32_t(0), (size_t)n + 1, rocprim::plus<uint32_t>(), ctx->stream));
	HIP_TRY(hipMemcpyAsync(total, koff + n, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
	return PCR_OK;
}

// Where end3_batches leaves what it computes: the caller's arrays on the host (pcr_pool_dimers_end3), or `dense` on the device
// (pcr_pool_conflicts_ext): n*n cell records, cell c = q*n + t at [c], every cell's final record whether or not the filter
// keeps it (a cell without placements: its ids, n_duplexes and PCR_DIMER_HOMO, zero elsewhere).  With dense the batch's records
// are merged in place there; nothing is kept, compacted or downloaded and no placement is listed.
struct End3Out {
	pcr_pool_dimer_end3 *out = nullptr; uint64_t cap = 0;
	pcr_dimer_placement *place_out = nullptr; uint64_t place_cap = 0;
	pcr_pool_dimer_end3 *dense = nullptr;
};

// The batch loop of pcr_pool_dimers_end3 over the n*n cells of the plan H (n > 0; the caller has checked the arguments, flushed
// the handle and set the device): scan<false>, scan, cells, scan<true>, melt, merge, keep / compact.  who begins the messages.
// kept_total = the kept cells, place_total = the kept placements (both 0 with O.dense).
int end3_batches(const char *who, pcr_ctx *ctx, const DimerHostPlan &H, const pcr_thermo_args *args, uint32_t min_run, uint32_t min_extension,
	float dg_max, const End3Out &O, uint64_t &kept_total, uint64_t &place_total)
{
	pcr_pool_dimer_end3 *const out = O.out;
	pcr_dimer_placement *const place_out = O.place_out;
	const uint64_t cap = O.cap, place_cap = O.place_cap;
	const bool dense = O.dense != nullptr;
	const uint32_t n = H.n;
	const uint64_t n_cells = (uint64_t)n*n;
	const bool keep_all = dg_max == INFINITY;
	// ---- the tables
	int rc;
	std::vector<uint8_t> blob;
	DimerPlan P;
	if((rc = pdim_upload_plan(ctx, H, blob, P)) != PCR_OK) return rc;
	if((rc = ctx->pdim_flag.ensure(1)) != PCR_OK) return rc;
	HIP_TRY(hipMemsetAsync(ctx->pdim_flag.p, 0, sizeof(uint32_t), ctx->stream));
	bool tables = false;                                                          // the dG table and the kernel's LDS size: only once something is melted
	// duplexes before cell c (c = n_cells: all of them)
	auto before = [&](uint64_t c) -> uint32_t {
		if(c >= n_cells) return H.row[n];
		const uint32_t q = (uint32_t)(c/n), t = (uint32_t)(c % n);
		return pdim_before(H.row.data(), H.pref.data(), q, t, H.ol[q].n_exp);
	};
	const float log_na = logf(args->salt);
	uint64_t c0 = 0;
	kept_total = place_total = 0;
	bool cells_live = cap > 0, place_live = place_cap > 0;                         // still within the caller's arrays
	while(c0 < n_cells){
		// ---- a batch: cells c0 .. c1 - 1; it closes before the cell that would take it past POOL_DIMER_END3_BATCH_DUPLEXES duplexes
		const uint32_t d0 = before(c0);
		uint64_t c1 = c0 + 1, above = n_cells + 1;
		while(above - c1 > 1){
			const uint64_t mid = c1 + (above - c1)/2;
			if(before(mid) - d0 <= POOL_DIMER_END3_BATCH_DUPLEXES) c1 = mid; else above = mid;
		}
		const uint32_t nd = before(c1) - d0, nc = (uint32_t)(c1 - c0);
		const size_t n_keep = (size_t)std::max(nc, POOL_DIMER_END3_BATCH_JOBS) + 1;
		if((rc = ctx->pde3_cnt.ensure((size_t)nd + 1)) != PCR_OK) return rc;
		if((rc = ctx->pde3_off.ensure((size_t)nd + 1)) != PCR_OK) return rc;
		if(!dense && (rc = ctx->pde3_rec.ensure(nc)) != PCR_OK) return rc;
		pcr_pool_dimer_end3 *const rec = dense ? O.dense + c0 : ctx->pde3_rec.p;     // the batch's cell records
		if((rc = ctx->pde3_keep.ensure(n_keep)) != PCR_OK) return rc;
		if((rc = ctx->pde3_koff.ensure(n_keep)) != PCR_OK) return rc;
		// ---- count, scan
		const unsigned grid_d = (unsigned)(((uint64_t)nd*32u + POOL_THREADS - 1)/POOL_THREADS), grid_c = (nc + POOL_THREADS - 1)/POOL_THREADS;
		hipLaunchKernelGGL(k_dimer_end3_scan<false>, dim3(grid_d), dim3(POOL_THREADS), 0, ctx->stream, P, (uint32_t)c0, d0, nd, min_run, min_extension,
			ctx->pde3_cnt.p, (const uint32_t *)nullptr, (uint2 *)nullptr);
		HIP_TRY(hipGetLastError());
		uint32_t n_jobs = 0;
		if((rc = end3_scan(ctx, ctx->pde3_cnt.p, ctx->pde3_off.p, nd, &n_jobs)) != PCR_OK) return rc;
		hipLaunchKernelGGL(k_dimer_end3_cells, dim3(grid_c), dim3(POOL_THREADS), 0, ctx->stream, P, (uint32_t)c0, nc, d0, (const uint32_t *)ctx->pde3_off.p, rec);
		HIP_TRY(hipGetLastError());
		HIP_TRY(hipStreamSynchronize(ctx->stream));
		// ---- fill and melt, while anything still needs the energies
		const bool melt = n_jobs && (!keep_all || cells_live || place_live || dense);
		if(melt){
			if(!tables){
				if((rc = ensure_dg_table(ctx, args->salt)) != PCR_OK) return rc;
				if(!ctx->pde3_attr_set){
					HIP_TRY(hipFuncSetAttribute((const void *)k_dimer_end3_melt, hipFuncAttributeMaxDynamicSharedMemorySize, (int)PDIM_LDS));
					ctx->pde3_attr_set = true;
				}
				tables = true;
			}
			if((rc = ctx->pde3_jobs.ensure(n_jobs)) != PCR_OK) return rc;
			if((rc = ctx->pde3_res.ensure(std::min(n_jobs, POOL_DIMER_END3_BATCH_JOBS))) != PCR_OK) return rc;
			hipLaunchKernelGGL(k_dimer_end3_scan<true>, dim3(grid_d), dim3(POOL_THREADS), 0, ctx->stream, P, (uint32_t)c0, d0, nd, min_run, min_extension,
				(uint32_t *)nullptr, (const uint32_t *)ctx->pde3_off.p, ctx->pde3_jobs.p);
			HIP_TRY(hipGetLastError());
			for(uint32_t a = 0;a < n_jobs;a += POOL_DIMER_END3_BATCH_JOBS){
				const uint32_t nj = std::min(POOL_DIMER_END3_BATCH_JOBS, n_jobs - a);
				// at most one block per CU (a block takes most of a CU's LDS), the waves striding over the jobs
				const unsigned grid_j = std::max(1u, std::min<unsigned>((nj + PDIM_WAVES - 1)/PDIM_WAVES, (unsigned)ctx->n_cu));
				hipLaunchKernelGGL(k_dimer_end3_melt, dim3(grid_j), dim3(PDIM_THREADS), PDIM_LDS, ctx->stream, P, (uint32_t)c0, (const uint2 *)(ctx->pde3_jobs.p + a), nj,
					(const int *)ctx->th_dg.p, log_na, ctx->pde3_res.p);
				HIP_TRY(hipGetLastError());
				hipLaunchKernelGGL(k_dimer_end3_merge, dim3(grid_c), dim3(POOL_THREADS), 0, ctx->stream, P, (uint32_t)c0, nc, d0, (const uint32_t *)ctx->pde3_off.p,
					(const uint2 *)ctx->pde3_jobs.p, a, nj, (const float4 *)ctx->pde3_res.p, rec, ctx->pdim_flag.p);
				HIP_TRY(hipGetLastError());
				uint32_t pk = nj;
				if(dense) continue;                                                     // (no placement is listed or counted)
				if(!keep_all || place_live){
					// ---- the launch's kept placements, in job order
					const unsigned grid_p = (nj + POOL_THREADS - 1)/POOL_THREADS;
					hipLaunchKernelGGL(k_dimer_end3_place_keep, dim3(grid_p), dim3(POOL_THREADS), 0, ctx->stream, (const float4 *)ctx->pde3_res.p, nj, dg_max, ctx->pde3_keep.p);
					HIP_TRY(hipGetLastError());
					if((rc = end3_scan(ctx, ctx->pde3_keep.p, ctx->pde3_koff.p, nj, &pk)) != PCR_OK) return rc;
					HIP_TRY(hipStreamSynchronize(ctx->stream));
					if(place_live && place_total + pk > place_cap) place_live = false;   // (past place_cap the call only counts)
					if(place_live && pk){
						if((rc = ctx->pde3_place.ensure(pk)) != PCR_OK) return rc;
						hipLaunchKernelGGL(k_dimer_end3_place_write, dim3(grid_p), dim3(POOL_THREADS), 0, ctx->stream, P, (uint32_t)c0, (const uint2 *)(ctx->pde3_jobs.p + a),
							(const float4 *)ctx->pde3_res.p, (const uint32_t *)ctx->pde3_keep.p, (const uint32_t *)ctx->pde3_koff.p, nj, ctx->pde3_place.p);
						HIP_TRY(hipGetLastError());
						HIP_TRY(hipMemcpyAsync(place_out + place_total, ctx->pde3_place.p, (size_t)pk*sizeof(pcr_dimer_placement), hipMemcpyDeviceToHost, ctx->stream));
						HIP_TRY(hipStreamSynchronize(ctx->stream));                     // the next launch reuses the scratch
					}
				}
				place_total += pk;
			}
		}
		else place_total += n_jobs;                                                 // (dg_max = +INFINITY keeps every qualifying placement)
		if(dense){
			uint32_t bad = 0;
			HIP_TRY(hipMemcpyAsync(&bad, ctx->pdim_flag.p, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
			HIP_TRY(hipStreamSynchronize(ctx->stream));                               // the next batch reuses the scratch
			if(bad & 1u){ g_err = std::string(who) + ": internal trace-back error"; return PCR_ERR_RANGE; }
			c0 = c1;
			continue;
		}
		// ---- the kept cells, in cell order
		hipLaunchKernelGGL(k_dimer_end3_cell_keep, dim3(grid_c), dim3(POOL_THREADS), 0, ctx->stream, (const pcr_pool_dimer_end3 *)rec, nc, keep_all ? 1 : 0, dg_max,
			ctx->pde3_keep.p);
		HIP_TRY(hipGetLastError());
		uint32_t kept = 0, bad = 0;
		if((rc = end3_scan(ctx, ctx->pde3_keep.p, ctx->pde3_koff.p, nc, &kept)) != PCR_OK) return rc;
		HIP_TRY(hipMemcpyAsync(&bad, ctx->pdim_flag.p, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
		HIP_TRY(hipStreamSynchronize(ctx->stream));
		if(bad & 1u){ g_err = std::string(who) + ": internal trace-back error"; return PCR_ERR_RANGE; }
		if(cells_live && kept_total + kept > cap) cells_live = false;               // (past cap the call only counts)
		if(cells_live && kept){
			if((rc = ctx->pde3_out.ensure(kept)) != PCR_OK) return rc;
			hipLaunchKernelGGL(k_dimer_end3_cell_compact, dim3(grid_c), dim3(POOL_THREADS), 0, ctx->stream, (const pcr_pool_dimer_end3 *)rec,
				(const uint32_t *)ctx->pde3_keep.p, (const uint32_t *)ctx->pde3_koff.p, nc, ctx->pde3_out.p);
			HIP_TRY(hipGetLastError());
			HIP_TRY(hipMemcpyAsync(out + kept_total, ctx->pde3_out.p, (size_t)kept*sizeof(pcr_pool_dimer_end3), hipMemcpyDeviceToHost, ctx->stream));
			HIP_TRY(hipStreamSynchronize(ctx->stream));                               // the next batch reuses the scratch
		}
		kept_total += kept;
		c0 = c1;
	}
	if(dense) place_total = 0;
	return PCR_OK;
}

} // namespace

extern "C" {

int64_t pcr_pool_dimers_end3(pcr_ctx *ctx, const pcr_pair *pool, uint32_t n_pool, const pcr_thermo_args *args, int rule,
	uint32_t min_run, uint32_t min_extension, float dg_max, uint32_t *oligo_id,
	pcr_pool_dimer_end3 *out, uint64_t cap, pcr_dimer_placement *place_out, uint64_t place_cap, uint64_t *n_place)
{
	static_assert(sizeof(pcr_pool_dimer_end3) == 48 && sizeof(pcr_dimer_placement) == 40, "record layout");
	// ---- the arguments, before the handle
	if(!args || (n_pool && (!pool || !oligo_id)) || (cap && !out) || (place_cap && !place_out)){ g_err = "pcr_pool_dimers_end3: bad argument"; return PCR_ERR_ARG; }
	if(n_pool > PCR_POOL_MAX_PAIRS){ g_err = "pcr_pool_dimers_end3: pool larger than PCR_POOL_MAX_PAIRS"; return PCR_ERR_ARG; }
	if(rule != PCR_DIMER_RULE_POOL && rule != PCR_DIMER_RULE_ASSAY){ g_err = "pcr_pool_dimers_end3: unknown rule (PCR_DIMER_RULE_POOL or PCR_DIMER_RULE_ASSAY)"; return PCR_ERR_ARG; }
	if(!(args->primer_strand > 0.0f)){ g_err = "pcr_pool_dimers_end3: primer_strand must be positive (NucCruc::strand, nuc_cruc.h:818-826)"; return PCR_ERR_ARG; }
	if(!(args->salt >= 1.0e-6f && args->salt <= 1.0f)){ g_err = "pcr_pool_dimers_end3: salt outside [1e-6, 1] (NucCruc::salt, nuc_cruc.h:780-788)"; return PCR_ERR_ARG; }
	if(min_run < 3u || min_run > 32u){ g_err = "pcr_pool_dimers_end3: min_run outside 3 .. 32 (the engine gives no energy to a duplex of 1 or 2 bases)"; return PCR_ERR_ARG; }
	if(min_extension > 31u){ g_err = "pcr_pool_dimers_end3: min_extension above 31"; return PCR_ERR_ARG; }
	if(dg_max != dg_max){ g_err = "pcr_pool_dimers_end3: dg_max is not a number"; return PCR_ERR_ARG; }
	DimerHostPlan H;
	{ const int prc = pdim_host_plan("pcr_pool_dimers_end3", pool, n_pool, args, rule, oligo_id, H); if(prc != PCR_OK) return prc; }
	if(!ctx){ g_err = "pcr_pool_dimers_end3: null handle"; return PCR_ERR_ARG; }
	FLUSH(ctx);
	HIP_TRY(hipSetDevice(ctx->device));
	if(n_place) *n_place = 0;
	if(H.n == 0) return 0;
	End3Out O;
	O.out = out; O.cap = cap; O.place_out = place_out; O.place_cap = place_cap;
	uint64_t kept_total = 0, place_total = 0;
	{ const int brc = end3_batches("pcr_pool_dimers_end3", ctx, H, args, min_run, min_extension, dg_max, O, kept_total, place_total); if(brc != PCR_OK) return brc; }
	if(n_place) *n_place = place_total;
	return (int64_t)kept_total;
}

} // extern "C"
