// Every oligo-by-oligo dimer of a primer pool (pcr_pool_dimers; included by pcr_device.hip after pcr_site_tm.inc, whose odometer
// rank it shares).
//
// A cell is an ORDERED pair (query oligo, target oligo) of the pool's distinct oligos; its duplexes are (expansion of the query)
// x (expansion of the target), off the diagonal NucCruc's heterodimer, on the diagonal one homodimer per expansion -- the
// definition is written out at pcr_pool_dimers in include/pcramp_hip.h.  Nothing is spelt on the host:
//   1. The host numbers the oligos, uploads one 32-byte record each (slot masks, ends, expansions, degeneracy class), two prefix
//      arrays (pref[t] = expansions of the oligos before t; row[q] = duplexes of the rows before q) and the log strand
//      concentration per pair of degeneracy classes -- D takes few values, no logf per cell.
//   2. k_pool_dimer: one wave per duplex, grid-strided, THERMO_WAVES independent waves per block around one LDS copy of the dG
//      table -- k_site_tm's shape, for k_site_tm's reason.  The wave derives (row, column, query expansion, target expansion) from
//      its job number by two guided searches over row[] and pref[] (the diagonal cell is D(q) duplexes, not D(q)^2: one correction),
//      its lanes spell both strands from the oligos' slot masks (pdim_code: the digit of a slot in the odometer of Word::begin()
//      / next()), and it runs Engine<1>::fill_wave -> collect_rows -> enumerate_parallel<false>(homo = diagonal).  No thermo::Job
//      exists.
//   3. k_pool_dimer_reduce, a thread per cell, walks the cell's duplexes in index order (max, min, lowest index on a tie: no
//      float atomics); an exclusive scan over the keep flags and k_pool_dimer_compact put the cells with tm_max >= tm_floor into
//      cell order.
// Per-duplex results are scratch, so the call runs in batches of consecutive whole cells of at most POOL_DIMER_BATCH_JOBS
// duplexes.  The call owns its scratch (pcr_ctx::pdim_*); the dG table is the handle's (th_dg, keyed by its salt).

namespace {

constexpr uint32_t POOL_DIMER_BATCH_JOBS = 1u << 21;                            // mirrored in api.py; 32 MB of float4 (DESIGN.md has the bound)
constexpr int PDIM_WAVES = thermo::THERMO_WAVES;
constexpr int PDIM_THREADS = 64*PDIM_WAVES;
constexpr size_t PDIM_LDS = thermo::THERMO_LDS;
constexpr uint32_t PDIM_ST_ERROR = 1u;                                          // bit of a duplex's status word
static_assert(POOL_DIMER_BATCH_JOBS >= 65536u, "a batch holds the largest cell (PCR_SITE_MAX_EXPANSIONS squared)");
static_assert((uint64_t)PCR_SITE_MAX_EXPANSIONS*PCR_SITE_MAX_EXPANSIONS <= 65536u, "a cell stays within pcr_dimer's 65 536 duplexes");

struct DimerOligo { Planes m; int32_t start, stop; uint32_t n_exp, cls; };      // slot masks, Word::start() / stop(), degeneracy, its class

// what the kernels read: n oligos; pref[0 .. n], row[0 .. n]; log strand by (class of q)*n_cls + (class of t), and by class on the diagonal
struct DimerPlan { const DimerOligo *ol; const uint32_t *pref, *row; const float *log_off, *log_diag; uint32_t n, n_cls; };

// duplexes before cell (q, t): the rows before q, the cells before t in row q, and the diagonal cell counted as D(q), not D(q)^2
__host__ __device__ inline uint32_t pdim_before(const uint32_t *row, const uint32_t *pref, uint32_t q, uint32_t t, uint32_t dq)
{
	return row[q] + dq*pref[t] - ((t > q) ? dq*dq - dq : 0u);
}

// The largest i in 0 .. n - 1 with a[i] <= x (a[0] = 0), looked for around `guess`: steps of 1, 2, 4, .. away from it until x is
// bracketed, then a bisection of the bracket.  Every load here is one more in a chain of dependent ones a wave waits out before
// its DP starts; a guess that is right, or a few entries off, ends the chain after two or three instead of eleven.
__device__ __forceinline__ unsigned pdim_floor_near(const uint32_t *__restrict__ a, unsigned n, unsigned x, unsigned guess)
{
	unsigned lo = min(guess, n - 1u), above, step = 1;
	if(a[lo] <= x){
		while(lo + step < n && a[lo + step] <= x){ lo += step; step *= 2u; }
		above = min(lo + step, n);
	}
	else{
		above = lo;                                                                // a[above] > x, above >= 1
		while(above > step && a[above - step] > x){ above -= step; step *= 2u; }
		lo = (above > step) ? above - step : 0u;
	}
	while(above - lo > 1u){                                                        // a[lo] <= x < a[above] (above = n: no upper entry)
		const unsigned mid = lo + (above - lo)/2u;
		if(a[mid] <= x) lo = mid; else above = mid;
	}
	return lo;
}

// The base code of slot s in expansion `expansion` of the oligo with slot masks m: the expansion index is a mixed-radix number
// over the degenerate slots in the odometer's order (site_rank: slot 15 fastest, then 14 .. 0, then 31 .. 16), a digit picks
// among the slot's bases, lowest first.  Both strands of a duplex are spelt with it.
__device__ __forceinline__ unsigned char pdim_code(const Planes &m, unsigned s, unsigned expansion, unsigned n_exp)
{
	auto base_set = [&](unsigned k) -> unsigned { return ((m.a >> k) & 1u) | (((m.c >> k) & 1u) << 1) | (((m.g >> k) & 1u) << 2) | (((m.t >> k) & 1u) << 3); };
	if(n_exp == 1u){ const unsigned only = base_set(s); return (unsigned char)(only ? (unsigned)__ffs(only) - 1u : 0u); }   // a plain oligo has no digits (uniform per wave)
	const unsigned rk = site_rank(s);
	unsigned div = 1;
	for(unsigned p = 0;p < 32u;++p){
		const unsigned d = (unsigned)__popc(base_set(p));
		if(d > 1u && site_rank(p) < rk) div *= d;
	}
	unsigned set = base_set(s);
	const unsigned d = max((unsigned)__popc(set), 1u);
	for(unsigned skip = (expansion/div) % d;skip;--skip) set &= set - 1u;
	return (unsigned char)(set ? (unsigned)__ffs(set) - 1u : 0u);
}

// enumerate_parallel reports the winner's Tm only; its energies are still in the lanes' slabs: the same merge again (lowest
// dG, earliest cell on a tie) -> the winner's dH and dS, zeros where no lane has one.  There are three copies of this rule --
// the end of enumerate_parallel (pcr_thermo.inc), k_site_tm (pcr_site_tm.inc) and this one, which k_pool_dimer and
// k_dimer_end3_melt (pcr_pool_dimers_end3.inc) share: they must change together.
__device__ __forceinline__ void pdim_winner(const thermo::ParLane *par, float &dH, float &dS)
{
	using namespace thermo;
	int win = -1;
	float wdg = 0.0f;
	dH = dS = 0.0f;
	for(int l = 0;l < WAVE_PAR;++l){
		const ParLane &L = par[l];
		if(L.win < 0) continue;
		const float dgl = L.best.dH - TARGET_T*L.best.dS;
		if(win < 0 || dgl < wdg || (dgl == wdg && L.win < win)){ win = L.win; wdg = dgl; dH = L.best.dH; dS = L.best.dS; }
	}
}

// Duplex j (numbered over the whole matrix), j0 <= j < j0 + n_jobs: (tm, dH, dS, status) -> res[j - j0].
__global__ __launch_bounds__(PDIM_THREADS) void k_pool_dimer(DimerPlan P, uint32_t j0, uint32_t n_jobs, const int *__restrict__ dg_global, float log_na,
	float4 *__restrict__ res)
{
	using namespace thermo;
	extern __shared__ int pdim_lds[];                                             // dg [49*49] | PDIM_WAVES slabs
	int *const dg = pdim_lds;
	const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63u;
	WaveSlab &w = ((WaveSlab *)(pdim_lds + 49*49))[wave];
	for(int i = threadIdx.x;i < 49*49;i += PDIM_THREADS) dg[i] = dg_global[i];
	__syncthreads();                                                               // the only workgroup barrier
	Engine<1> e;
	e.dg = dg; e.log_na = log_na;
	e.q = w.q; e.t = w.t;
	e.mx.M = w.si;
	e.mx.tr = w.ss;
	const unsigned n_exp_all = P.pref[P.n];
	unsigned q = P.n;                                                              // the row of the wave's last job (none yet)
	for(unsigned jl = blockIdx.x*PDIM_WAVES + wave;jl < n_jobs;jl += gridDim.x*PDIM_WAVES){   // uniform per wave
		const unsigned j = j0 + jl;
		// row[q] <= j < row[q + 1]: at or a few rows after the last job's, j only grows; the first one by proportion
		q = pdim_floor_near(P.row, P.n, j, (q < P.n) ? q : (unsigned)((float)j*(float)P.n/(float)P.row[P.n]));
		const DimerOligo oq = P.ol[q];
		const unsigned dq = oq.n_exp, r = j - P.row[q], diag0 = dq*P.pref[q];
		const bool homo = r >= diag0 && r < diag0 + dq;
		unsigned t = q, iq = r - diag0, it = r - diag0;
		if(!homo){
			const unsigned rr = (r < diag0) ? r : r - dq + dq*dq;                   // as if the diagonal cell were D(q)^2 wide
			t = pdim_floor_near(P.pref, P.n, rr/dq, ((rr/dq)*P.n)/n_exp_all);   // (at most 2^19 * 2^11; exact where all oligos have as many expansions)
			const unsigned rem = rr - dq*P.pref[t], dt = P.ol[t].n_exp;
			iq = rem/dt; it = rem % dt;                                             // the reference's loops, query outer
		}
		const DimerOligo ot = P.ol[t];
		const int qlen = oq.stop - oq.start + 1, tlen = homo ? 0 : ot.stop - ot.start + 1;   // 1 .. 32 (the host refuses oligos with holes)
		e.log_strand = homo ? P.log_diag[oq.cls] : P.log_off[oq.cls*P.n_cls + ot.cls];
		e.qlen = qlen; e.tlen = tlen;                                               // (a homodimer has no target: k_thermo_wave's mode 2)
		if(lane <= MAXL){
			const int i = (int)lane;
			unsigned char qc = (unsigned char)bE, tc = (unsigned char)bE;           // "one past the end" is the non-pairing code E
			if(i < qlen) qc = pdim_code(oq.m, (unsigned)(oq.start + i), iq, dq);
			if(i < tlen) tc = pdim_code(ot.m, (unsigned)(ot.start + i), it, ot.n_exp);
			w.q[i] = qc; w.t[i] = tc;
		}
		wave_sync();
		const int TL = homo ? qlen : tlen;
		const int mxs = e.fill_wave(e.q, e.qlen, homo ? e.q : e.t, e.qlen, TL, 0);
		wave_sync();
		collect_rows(e, e.qlen, TL, 0, mxs, w.rowmask);
		wave_sync();
		unsigned status = 0;
		const float tm = enumerate_parallel<false>(e, w.par, w.rowmask, e.qlen, homo, status);
		if(lane == 0){
			float dH, dS;
			pdim_winner(w.par, dH, dS);
			res[jl] = make_float4(tm, dH, dS, __uint_as_float((status & 1u) ? PDIM_ST_ERROR : 0u));
		}
		wave_sync();                                                               // before the next job overwrites the sequences
	}
}

// Cell c0 + k, k < n_cells: its duplexes in index order; the highest Tm (the lowest index on a tie) gives the expansions, dH and dS.
__global__ __launch_bounds__(POOL_THREADS) void k_pool_dimer_reduce(DimerPlan P, uint32_t c0, uint32_t n_cells, uint32_t j0, const float4 *__restrict__ res,
	float tm_floor, pcr_pool_dimer *__restrict__ rec, uint32_t *__restrict__ keep, uint32_t *__restrict__ error)
{
	const uint32_t k = blockIdx.x*blockDim.x + threadIdx.x;
	if(k >= n_cells) return;
	const uint32_t c = c0 + k, q = c/P.n, t = c % P.n;
	const uint32_t dq = P.ol[q].n_exp, dt = P.ol[t].n_exp;
	const bool homo = (q == t);
	const uint32_t nd = homo ? dq : dq*dt, first = pdim_before(P.row, P.pref, q, t, dq) - j0;
	pcr_pool_dimer d;
	d.query_oligo = q; d.target_oligo = t; d.n_duplexes = nd; d.flags = homo ? PCR_DIMER_HOMO : 0u;
	d.tm_max = d.tm_min = d.dH = d.dS = 0.0f;
	uint32_t st = 0, best = 0;
	for(uint32_t i = 0;i < nd;++i){
		const float4 v = res[first + i];
		st |= __float_as_uint(v.w);
		if(i == 0 || v.x > d.tm_max){ d.tm_max = v.x; d.dH = v.y; d.dS = v.z; best = i; }
		if(i == 0 || v.x < d.tm_min) d.tm_min = v.x;
	}
	d.q_expansion = homo ? best : best/dt; d.t_expansion = homo ? best : best % dt;
	if(st & PDIM_ST_ERROR) atomicOr(error, 1u);
	rec[k] = d;
	keep[k] = (!(tm_floor > 0.0f) || d.tm_max >= tm_floor) ? 1u : 0u;
}

// the kept cells, in cell order: off = exclusive scan of keep
__global__ __launch_bounds__(POOL_THREADS) void k_pool_dimer_compact(const pcr_pool_dimer *__restrict__ rec, const uint32_t *__restrict__ keep,
	const uint32_t *__restrict__ off, uint32_t n_cells, pcr_pool_dimer *__restrict__ out)
{
	const uint32_t k = blockIdx.x*blockDim.x + threadIdx.x;
	if(k < n_cells && keep[k]) out[off[k]] = rec[k];
}

// What the host works out from a pool before it looks at the handle (pcr_pool_dimers and pcr_pool_dimers_end3 refuse the same
// pools in the same order, `who` begins the message): the distinct oligos in order of first appearance, the two prefix arrays
// and the log strand concentration of every pair of degeneracy classes.
struct DimerHostPlan { std::vector<DimerOligo> ol; std::vector<uint32_t> pref, row; std::vector<float> logs; uint32_t n = 0, n_cls = 0; };

int pdim_host_plan(const char *who, const pcr_pair *pool, uint32_t n_pool, const pcr_thermo_args *args, int rule, uint32_t *oligo_id, DimerHostPlan &H)
{
	const std::string w = std::string(who) + ": ";
	// the distinct oligos, in order of first appearance (as pcr_pool_products)
	std::vector<DimerOligo> &ol = H.ol;
	std::vector<uint32_t> cls_degen;                                              // the distinct degeneracies
	std::map<std::pair<uint64_t, uint64_t>, uint32_t> id_of;
	for(uint32_t s = 0;s < 2*n_pool;++s){
		const pcr_word128 &wd = (s & 1) ? pool[s/2].r : pool[s/2].f;
		auto ins = id_of.insert(std::make_pair(std::make_pair(wd.w[0], wd.w[1]), (uint32_t)ol.size()));
		if(ins.second){
			DimerOligo d;
			d.m = pcrhost::planes_of_word(wd.w);
			d.start = pcrhost::planes_start(d.m); d.stop = pcrhost::planes_stop(d.m);
			const uint32_t occ = pcrhost::planes_occupied(d.m);
			if(!occ || __builtin_popcount(occ) != d.stop - d.start + 1){
				g_err = w + "an oligo is empty or has a hole between its ends (NucCruc::set_query throws)"; return PCR_ERR_ARG;
			}
			const double degen = pcrhost::planes_degeneracy(d.m);
			if(degen > (double)PCR_SITE_MAX_EXPANSIONS){ g_err = w + "an oligo has more than PCR_SITE_MAX_EXPANSIONS expansions"; return PCR_ERR_ARG; }
			d.n_exp = (uint32_t)degen;
			const auto at = std::find(cls_degen.begin(), cls_degen.end(), d.n_exp);
			d.cls = (uint32_t)(at - cls_degen.begin());
			if(at == cls_degen.end()) cls_degen.push_back(d.n_exp);
			ol.push_back(d);
		}
		oligo_id[s] = ins.first->second;
	}
	const uint32_t n = H.n = (uint32_t)ol.size(), n_cls = H.n_cls = (uint32_t)cls_degen.size();
	std::vector<uint32_t> &pref = H.pref, &row = H.row;
	pref.assign(n + 1, 0); row.assign(n + 1, 0);
	for(uint32_t t = 0;t < n;++t) pref[t + 1] = pref[t] + ol[t].n_exp;            // at most 2 048 * 256
	{
		uint64_t total = 0;
		for(uint32_t q = 0;q < n;++q){
			row[q] = (uint32_t)total;
			total += (uint64_t)ol[q].n_exp*(pref[n] - ol[q].n_exp) + ol[q].n_exp;
			if(total >= (uint64_t(1) << 31)){ g_err = w + "the pool's duplexes number 2^31 or more"; return PCR_ERR_CAPACITY; }
		}
		row[n] = (uint32_t)total;
	}
	// the log strand concentration of every pair of degeneracy classes (every log() on the host, as everywhere)
	std::vector<float> &logs = H.logs;
	logs.assign((size_t)n_cls*n_cls + n_cls, 0.0f);
	for(uint32_t a = 0;a < n_cls;++a){
		const float ca = (float)(args->primer_strand/(double)cls_degen[a]);
		for(uint32_t b = 0;b < n_cls;++b){
			const float cb = (float)(args->primer_strand/(double)cls_degen[b]);
			const float strand = (rule == PCR_DIMER_RULE_POOL) ? args->primer_strand                    // pcr_assay.cpp:819-821
				: ((ca > cb) ? ca - 0.5f*cb : cb - 0.5f*ca);                                            // pcr_assay.cpp:244, nuc_cruc.h:832-837
			if(!(strand > 0.0f)){ g_err = w + "primer_strand / degeneracy underflows to zero"; return PCR_ERR_ARG; }
			logs[(size_t)a*n_cls + b] = logf(strand);
		}
		const float own = (rule == PCR_DIMER_RULE_POOL) ? args->primer_strand : ca;                     // valid_pcr.cpp:13
		if(!(own > 0.0f)){ g_err = w + "primer_strand / degeneracy underflows to zero"; return PCR_ERR_ARG; }
		logs[(size_t)n_cls*n_cls + a] = logf(own);
	}
	return PCR_OK;
}

// The plan's tables as one blob (the caller's, which must outlive the copy) into pdim_in, on the handle's stream -> what the kernels read.
int pdim_upload_plan(pcr_ctx *ctx, const DimerHostPlan &H, std::vector<uint8_t> &blob, DimerPlan &P)
{
	int rc;
	const size_t ol_bytes = (size_t)H.n*sizeof(DimerOligo), pre_bytes = (size_t)(H.n + 1)*sizeof(uint32_t), log_bytes = H.logs.size()*sizeof(float);
	blob.resize(ol_bytes + 2*pre_bytes + log_bytes);
	memcpy(blob.data(), H.ol.data(), ol_bytes);
	memcpy(blob.data() + ol_bytes, H.pref.data(), pre_bytes);
	memcpy(blob.data() + ol_bytes + pre_bytes, H.row.data(), pre_bytes);
	memcpy(blob.data() + ol_bytes + 2*pre_bytes, H.logs.data(), log_bytes);
	if((rc = ctx->pdim_in.ensure(blob.size())) != PCR_OK) return rc;
	HIP_TRY(hipMemcpyAsync(ctx->pdim_in.p, blob.data(), blob.size(), hipMemcpyHostToDevice, ctx->stream));
	P.ol = (const DimerOligo *)ctx->pdim_in.p;
	P.pref = (const uint32_t *)(ctx->pdim_in.p + ol_bytes);
	P.row = (const uint32_t *)(ctx->pdim_in.p + ol_bytes + pre_bytes);
	P.log_off = (const float *)(ctx->pdim_in.p + ol_bytes + 2*pre_bytes);
	P.log_diag = P.log_off + (size_t)H.n_cls*H.n_cls;
	P.n = H.n; P.n_cls = H.n_cls;
	return PCR_OK;
}

} // namespace

extern "C" {

int64_t pcr_pool_dimers(pcr_ctx *ctx, const pcr_pair *pool, uint32_t n_pool, const pcr_thermo_args *args, int rule,
	float tm_floor, uint32_t *oligo_id, pcr_pool_dimer *out, uint64_t cap)
{
	static_assert(sizeof(pcr_pool_dimer) == 40, "record layout");
	static_assert(sizeof(DimerOligo) == 32, "table layout");
	// ---- the arguments, before the handle
	if(!args || (n_pool && (!pool || !oligo_id)) || (cap && !out)){ g_err = "pcr_pool_dimers: bad argument"; return PCR_ERR_ARG; }
	if(n_pool > PCR_POOL_MAX_PAIRS){ g_err = "pcr_pool_dimers: pool larger than PCR_POOL_MAX_PAIRS"; return PCR_ERR_ARG; }
	if(rule != PCR_DIMER_RULE_POOL && rule != PCR_DIMER_RULE_ASSAY){ g_err = "pcr_pool_dimers: unknown rule (PCR_DIMER_RULE_POOL or PCR_DIMER_RULE_ASSAY)"; return PCR_ERR_ARG; }
	if(!(args->primer_strand > 0.0f)){ g_err = "pcr_pool_dimers: primer_strand must be positive (NucCruc::strand, nuc_cruc.h:818-826)"; return PCR_ERR_ARG; }
	if(!(args->salt >= 1.0e-6f && args->salt <= 1.0f)){ g_err = "pcr_pool_dimers: salt outside [1e-6, 1] (NucCruc::salt, nuc_cruc.h:780-788)"; return PCR_ERR_ARG; }
	DimerHostPlan H;
	{ const int prc = pdim_host_plan("pcr_pool_dimers", pool, n_pool, args, rule, oligo_id, H); if(prc != PCR_OK) return prc; }
	const std::vector<DimerOligo> &ol = H.ol;
	const std::vector<uint32_t> &pref = H.pref, &row = H.row;
	const uint32_t n = H.n;
	if(!ctx){ g_err = "pcr_pool_dimers: null handle"; return PCR_ERR_ARG; }
	FLUSH(ctx);
	HIP_TRY(hipSetDevice(ctx->device));
	if(n == 0) return 0;
	const uint64_t n_cells = (uint64_t)n*n;
	const bool keep_all = !(tm_floor > 0.0f);
	if(keep_all && n_cells > cap) return (int64_t)n_cells;                        // count only: no thermodynamics needed, out is left as it is
	// ---- the tables
	int rc;
	std::vector<uint8_t> blob;
	DimerPlan P;
	if((rc = pdim_upload_plan(ctx, H, blob, P)) != PCR_OK) return rc;
	if((rc = ensure_dg_table(ctx, args->salt)) != PCR_OK) return rc;
	if(!ctx->pdim_attr_set){
		HIP_TRY(hipFuncSetAttribute((const void *)k_pool_dimer, hipFuncAttributeMaxDynamicSharedMemorySize, (int)PDIM_LDS));
		ctx->pdim_attr_set = true;
	}
	if((rc = ctx->pdim_flag.ensure(1)) != PCR_OK) return rc;
	HIP_TRY(hipMemsetAsync(ctx->pdim_flag.p, 0, sizeof(uint32_t), ctx->stream));
	// duplexes before cell c (c = n_cells: all of them)
	auto before = [&](uint64_t c) -> uint32_t {
		if(c >= n_cells) return row[n];
		const uint32_t q = (uint32_t)(c/n), t = (uint32_t)(c % n);
		return pdim_before(row.data(), pref.data(), q, t, ol[q].n_exp);
	};
	const float log_na = logf(args->salt);
	uint64_t kept_total = 0, c0 = 0;
	while(c0 < n_cells){
		// ---- a batch: cells c0 .. c1 - 1; it closes before the cell that would take it past POOL_DIMER_BATCH_JOBS duplexes
		const uint32_t j0 = before(c0);
		uint64_t c1 = c0 + 1, above = n_cells + 1;                                  // before(c1) - j0 <= the limit (one cell always is) < before(above) - j0
		while(above - c1 > 1){
			const uint64_t mid = c1 + (above - c1)/2;
			if(before(mid) - j0 <= POOL_DIMER_BATCH_JOBS) c1 = mid; else above = mid;
		}
		const uint32_t n_jobs = before(c1) - j0, nc = (uint32_t)(c1 - c0);
		if((rc = ctx->pdim_res.ensure(n_jobs)) != PCR_OK) return rc;
		if((rc = ctx->pdim_rec.ensure(nc)) != PCR_OK) return rc;
		if((rc = ctx->pdim_keep.ensure((size_t)nc + 1)) != PCR_OK) return rc;
		// at most one block per CU (a block takes most of a CU's LDS), the waves striding over the duplexes
		const unsigned grid_j = std::max(1u, std::min<unsigned>((n_jobs + PDIM_WAVES - 1)/PDIM_WAVES, (unsigned)ctx->n_cu));
		hipLaunchKernelGGL(k_pool_dimer, dim3(grid_j), dim3(PDIM_THREADS), PDIM_LDS, ctx->stream, P, j0, n_jobs, (const int *)ctx->th_dg.p, log_na, ctx->pdim_res.p);
		HIP_TRY(hipGetLastError());
		const unsigned grid_c = (nc + POOL_THREADS - 1)/POOL_THREADS;
		hipLaunchKernelGGL(k_pool_dimer_reduce, dim3(grid_c), dim3(POOL_THREADS), 0, ctx->stream, P, (uint32_t)c0, nc, j0, (const float4 *)ctx->pdim_res.p,
			tm_floor, ctx->pdim_rec.p, ctx->pdim_keep.p, ctx->pdim_flag.p);
		HIP_TRY(hipGetLastError());
		const pcr_pool_dimer *d_kept = ctx->pdim_rec.p;
		uint32_t kept = nc;
		if(!keep_all){
			// ---- the kept cells, in cell order
			if((rc = ctx->pdim_off.ensure((size_t)nc + 1)) != PCR_OK) return rc;
			HIP_TRY(hipMemsetAsync(ctx->pdim_keep.p + nc, 0, sizeof(uint32_t), ctx->stream));
			size_t tmp = 0;
			HIP_TRY(rocprim::exclusive_scan(nullptr, tmp, ctx->pdim_keep.p, ctx->pdim_off.p, uint32_t(0), (size_t)nc + 1, rocprim::plus<uint32_t>(), ctx->stream));
			if((rc = ctx->pdim_tmp.ensure(tmp + 16)) != PCR_OK) return rc;
			HIP_TRY(rocprim::exclusive_scan(ctx->pdim_tmp.p, tmp, ctx->pdim_keep.p, ctx->pdim_off.p, uint32_t(0), (size_t)nc + 1, rocprim::plus<uint32_t>(), ctx->stream));
			HIP_TRY(hipMemcpyAsync(&kept, ctx->pdim_off.p + nc, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
			HIP_TRY(hipStreamSynchronize(ctx->stream));
			if(kept && kept_total + kept <= cap){
				if((rc = ctx->pdim_out.ensure(kept)) != PCR_OK) return rc;
				hipLaunchKernelGGL(k_pool_dimer_compact, dim3(grid_c), dim3(POOL_THREADS), 0, ctx->stream, (const pcr_pool_dimer *)ctx->pdim_rec.p,
					(const uint32_t *)ctx->pdim_keep.p, (const uint32_t *)ctx->pdim_off.p, nc, ctx->pdim_out.p);
				HIP_TRY(hipGetLastError());
				d_kept = ctx->pdim_out.p;
			}
		}
		if(kept && kept_total + kept <= cap)                                        // (past cap the call only counts: out is unspecified then)
			HIP_TRY(hipMemcpyAsync(out + kept_total, d_kept, (size_t)kept*sizeof(pcr_pool_dimer), hipMemcpyDeviceToHost, ctx->stream));
		uint32_t bad = 0;
		HIP_TRY(hipMemcpyAsync(&bad, ctx->pdim_flag.p, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
		HIP_TRY(hipStreamSynchronize(ctx->stream));                                 // the next batch reuses the scratch
		if(bad & 1u){ g_err = "pcr_pool_dimers: internal trace-back error"; return PCR_ERR_RANGE; }
		kept_total += kept;
		c0 = c1;
	}
	return (int64_t)kept_total;
}

} // extern "C"
