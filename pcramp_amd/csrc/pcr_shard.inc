// The local search over targets sharded across ranks (include/pcramp_hip.h: pcr_shard_targets).  Included after
// pcr_exchange.inc, before the optimiser (pcr_optimize.inc), which calls the steps below.
//
// Only one target-dependent quantity reaches the optimiser's decisions: the target coverage of every trial word.  Trial words
// depend on the oligo alone, background / multiplex / oligo-overlap terms on sets every rank holds whole.  So a rank runs the
// unchanged move-coverage pass over ITS targets (its bitsets hold local sequence indices) and the ranks combine per trial word:
//   mode 1, exact partials: every rank sums its bits in double (k_cov_partial, both of compute_coverage's passes); ONE
//           all-gather of the per-rank sums; k_cov_combine adds them in rank order and casts to float.  Chosen at attach time
//           only where every partial sum is exactly representable (DESIGN.md section 7), so the order of the additions cannot
//           change the result;
//   mode 2, ordered chain: the reference's own sequential sum (pcr_assay.cpp:271-302) -- the {F(+),R(-)} pass over ranks
//           0..W-1, each continuing from the previous rank's double carry, then the {R(+),F(-)} pass over ranks 0..W-1 again:
//           2W all-gathers of one record per rank, of which the step's rank alone carries the sums.
// Every record starts with a status word: the has_split range error and any local failure become the same return code on
// every rank, and a rank that failed still takes part in every remaining collective.  Before each combine the ranks agree
// on the shape of the variant list (a header all-gather), and on entry to a sharded entry point on a fingerprint of the call.

namespace {

// ---- status words of the exchanged records
constexpr uint64_t SH_RANGE = 1ull;                 // Sequence::has_split out of bounds on some rank (sequence.cpp:306-308)
constexpr int SH_FAIL_SHIFT = 8;                    // bit SH_FAIL_SHIFT + (-rc): some rank failed with rc
inline uint64_t sh_fail_bit(int rc) { return (rc < 0 && rc >= -8) ? (1ull << (SH_FAIL_SHIFT - rc)) : (1ull << (SH_FAIL_SHIFT + 2)); }

// the agreed return code of a status word (the same on every rank); this rank's own message is kept when it failed itself
int sh_status_rc(uint64_t st, int local_rc, const char *what)
{
	if(!st) return PCR_OK;
	if(st & SH_RANGE){ g_err = "Sequence::has_split: range is out of bounds"; return PCR_ERR_RANGE; }
	for(int k = 1;k <= 8;++k){
		if(!(st & (1ull << (SH_FAIL_SHIFT + k)))) continue;
		if(local_rc != -k) g_err = std::string(what) + ": another rank failed";
		return -k;
	}
	g_err = std::string(what) + ": bad status word from a rank";
	return PCR_ERR_STATE;
}

inline uint64_t sh_hash(uint64_t h, const void *p, size_t bytes)        // FNV-1a, 64 bit
{
	const uint8_t *b = (const uint8_t *)p;
	for(size_t i = 0;i < bytes;++i){ h ^= b[i]; h *= 0x100000001B3ull; }
	return h;
}
constexpr uint64_t SH_HASH0 = 0xCBF29CE484222325ull;

// compute_coverage's weight sum (pcr_assay.cpp:280-301) over THIS rank's bits, continuing from carry[v] (nullptr: 0):
// phases bit 0 = the {F(+),R(-)} bits, bit 1 = the {R(+),F(-)} bits not yet counted -- k_cov_from_bits' walk, split so that
// the passes can run rank after rank.  rec[0] = the status word (flags | the has_split bit of the pass), rec[1 + v] = the
// double sum as its bits.  words = 0: this rank contributes the carry alone (no DB entries, or not its step of the chain).
__global__ void k_cov_partial(const uint64_t *__restrict__ bits_fr, const uint64_t *__restrict__ bits_rf, uint64_t words, const float *__restrict__ weights,
	uint64_t n_seq, uint32_t n_variants, const uint64_t *__restrict__ carry, uint32_t phases, const uint32_t *__restrict__ status, uint64_t flags,
	uint64_t *__restrict__ rec)
{
	const uint32_t v = blockIdx.x*blockDim.x + threadIdx.x;
	if(v == 0) rec[0] = flags | ((status && (status[0] & 1u)) ? SH_RANGE : 0ull);
	if(v >= n_variants) return;
	double ret = carry ? __longlong_as_double((long long)carry[v]) : 0.0;
	if(words){
		const uint64_t *fr = bits_fr + (size_t)v*words, *rf = bits_rf + (size_t)v*words;
		if(phases & 1u){
			for(uint64_t w = 0;w < words;++w){
				for(uint64_t m = fr[w];m;m &= m - 1){ const uint64_t i = w*64 + (uint64_t)(__ffsll((long long)m) - 1); if(i < n_seq) ret += weights[i]; }
			}
		}
		if(phases & 2u){
			for(uint64_t w = 0;w < words;++w){
				for(uint64_t m = rf[w] & ~fr[w];m;m &= m - 1){ const uint64_t i = w*64 + (uint64_t)(__ffsll((long long)m) - 1); if(i < n_seq) ret += weights[i]; }
			}
		}
	}
	rec[1 + v] = (uint64_t)__double_as_longlong(ret);
}

// the gathered records (rank r at full[r*stride]): cov[v] = (float) the sum over ranks [r_lo, r_hi) in rank order; *status_out =
// the OR of the status words of all `world` records
__global__ void k_cov_combine(const uint64_t *__restrict__ full, uint64_t stride, uint32_t r_lo, uint32_t r_hi, uint32_t world, uint32_t n_variants,
	float *__restrict__ cov, uint64_t *__restrict__ status_out)
{
	const uint32_t v = blockIdx.x*blockDim.x + threadIdx.x;
	if(v == 0){
		uint64_t st = 0;
		for(uint32_t r = 0;r < world;++r) st |= full[(size_t)r*stride];
		*status_out = st;
	}
	if(v >= n_variants) return;
	double s = 0.0;
	for(uint32_t r = r_lo;r < r_hi;++r) s += __longlong_as_double((long long)full[(size_t)r*stride + 1 + v]);
	cov[v] = (float)s;
}

// ---- all-gathers over either kind of communicator
// host memory in and out
int sh_allgather_host(pcr_ctx *ctx, pcr_comm *c, const void *send, uint64_t bytes, void *recv)
{
	if(c->host_fn){
		if(c->host_fn(send, bytes, recv, c->host_user) != 0){ g_err = "the host all-gather failed"; return PCR_ERR_DEVICE; }
		return PCR_OK;
	}
	RcclApi *api = rccl_api();
	if(!api) return PCR_ERR_STATE;
	int rc;
	if((rc = ctx->sh_stage.ensure((size_t)bytes*(c->world + 1))) != PCR_OK) return rc;
	HIP_TRY(hipMemcpyAsync(ctx->sh_stage.p, send, bytes, hipMemcpyHostToDevice, ctx->stream));
	RCCL_TRY(api, api->AllGather(ctx->sh_stage.p, ctx->sh_stage.p + bytes, (size_t)bytes, ncclUint8, c->comm, ctx->stream));
	HIP_TRY(hipMemcpyAsync(recv, ctx->sh_stage.p + bytes, (size_t)bytes*c->world, hipMemcpyDeviceToHost, ctx->stream));
	HIP_TRY(hipStreamSynchronize(ctx->stream));
	return PCR_OK;
}

// a record of `words` u64 (status word first) on the device, gathered into d_full (world x words) in stream order.  On a host
// communicator a rank whose copy to the host fails still sends: a record of zeros carrying the failure in its status word.
int sh_allgather_rec(pcr_ctx *ctx, pcr_comm *c, const uint64_t *d_rec, uint64_t words, uint64_t *d_full)
{
	if(c->host_fn){
		std::vector<uint64_t> send(words, 0), recv((size_t)words*c->world);
		hipError_t e = hipMemcpyAsync(send.data(), d_rec, words*sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream);
		if(e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
		if(e != hipSuccess){ std::fill(send.begin(), send.end(), 0ull); send[0] = sh_fail_bit(PCR_ERR_DEVICE); }
		if(c->host_fn(send.data(), words*sizeof(uint64_t), recv.data(), c->host_user) != 0){ g_err = "the host all-gather failed"; return PCR_ERR_DEVICE; }
		if(e != hipSuccess){ g_err = std::string("shard record: ") + hipGetErrorString(e); return PCR_ERR_DEVICE; }
		HIP_TRY(hipMemcpyAsync(d_full, recv.data(), recv.size()*sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
		HIP_TRY(hipStreamSynchronize(ctx->stream));                               // (recv is about to go away)
		return PCR_OK;
	}
	RcclApi *api = rccl_api();
	if(!api) return PCR_ERR_STATE;
	RCCL_TRY(api, api->AllGather(d_rec, d_full, (size_t)words, ncclUint64, c->comm, ctx->stream));
	return PCR_OK;
}

// ---- agreement steps
// On entry to a sharded entry point: every rank's status and fingerprint of the call, over `c` (nullptr: the attached shard's
// communicator).  Returns the same code on every rank: a local failure anywhere, or PCR_ERR_ARG when the fingerprints differ.
int shard_agree(pcr_ctx *ctx, uint64_t fingerprint, int local_rc, const char *what, pcr_comm *c = nullptr)
{
	if(!c) c = ctx->shard_comm;
	const uint64_t me[2] = {local_rc != PCR_OK ? sh_fail_bit(local_rc) : 0ull, fingerprint};
	std::vector<uint64_t> all(2*(size_t)c->world);
	const int rc = sh_allgather_host(ctx, c, me, sizeof(me), all.data());
	if(rc != PCR_OK) return rc;
	uint64_t st = 0; bool same = true;
	for(int r = 0;r < c->world;++r){ st |= all[2*(size_t)r]; same = same && all[2*(size_t)r + 1] == fingerprint; }
	if(st) return sh_status_rc(st, local_rc, what);
	if(!same){ g_err = std::string(what) + ": the ranks were given different batches (assays, arguments or pool)"; return PCR_ERR_ARG; }
	return PCR_OK;
}

// Before an iteration's target combine: the status of everything the rank did so far in the iteration and the shape of its
// variant list (count and a hash of the per-oligo ranges).  The combine's buffers are allocated first, so that nothing after
// this step can fail without the other ranks hearing of it.  nv = 0 with local_rc != PCR_OK: a rank that failed before it had a list.
int shard_header(pcr_ctx *ctx, int local_rc, uint64_t nv, uint64_t shape)
{
	pcr_comm *c = ctx->shard_comm;
	if(local_rc == PCR_OK && nv){
		local_rc = ctx->sh_rec.ensure((size_t)nv + 2);
		if(local_rc == PCR_OK) local_rc = ctx->sh_full.ensure(((size_t)nv + 1)*c->world);
		if(local_rc == PCR_OK) local_rc = ctx->opt_cov.ensure((size_t)nv + 4);
	}
	const uint64_t me[3] = {local_rc != PCR_OK ? sh_fail_bit(local_rc) : 0ull, nv, shape};
	std::vector<uint64_t> all(3*(size_t)c->world);
	const int rc = sh_allgather_host(ctx, c, me, sizeof(me), all.data());
	if(rc != PCR_OK) return rc;
	uint64_t st = 0; bool same = true;
	for(int r = 0;r < c->world;++r){ st |= all[3*(size_t)r]; same = same && all[3*(size_t)r + 1] == nv && all[3*(size_t)r + 2] == shape; }
	if(st) return sh_status_rc(st, local_rc, "pcr_optimize_batch");
	if(!same){ g_err = "pcr_optimize_batch: the ranks' trial word lists differ"; return PCR_ERR_STATE; }
	return PCR_OK;
}

// The combine of one target coverage pass: this rank's bitsets (bits_fr / bits_rf of `words` words per variant, local sequence
// indices; words = 0: none) -> cov_out[v] for all nv variants, identical on every rank.  local_rc: the pass's own outcome.
int shard_combine(pcr_ctx *ctx, SeqSet &S, uint32_t nv, uint64_t words, bool have_status, int local_rc, std::vector<float> &cov_out)
{
	pcr_comm *c = ctx->shard_comm;
	const uint32_t W = (uint32_t)c->world, me = (uint32_t)c->rank;
	const uint64_t stride = (uint64_t)nv + 1;
	uint64_t flags = local_rc != PCR_OK ? sh_fail_bit(local_rc) : 0ull;
	if(local_rc != PCR_OK){ words = 0; have_status = false; }
	int rc_comm = PCR_OK;
	auto partial = [&](uint32_t n_var, const uint64_t *carry, uint32_t phases){
		hipLaunchKernelGGL(k_cov_partial, dim3(std::max(1u, (n_var + 127)/128)), dim3(128), 0, ctx->stream, ctx->bits_fr.p, ctx->bits_rf.p, words, S.d_weight.p,
			(uint64_t)S.n, n_var, carry, phases, have_status ? (const uint32_t *)ctx->status.p : nullptr, flags, ctx->sh_rec.p);
		const hipError_t e = hipGetLastError();
		if(e != hipSuccess && !(flags & ~SH_RANGE)){ g_err = std::string("k_cov_partial: ") + hipGetErrorString(e); local_rc = PCR_ERR_DEVICE; flags |= sh_fail_bit(PCR_ERR_DEVICE); }
	};
	auto gather = [&](){
		if(rc_comm != PCR_OK) return;                                             // (a broken transport: nothing more can be exchanged)
		rc_comm = sh_allgather_rec(ctx, c, ctx->sh_rec.p, stride, ctx->sh_full.p);
	};
	uint32_t r_lo = 0, r_hi = W;
	if(ctx->shard_mode == 1){
		partial(nv, nullptr, 3u);
		gather();
	}
	else{
		// the chain: rank r's step continues from rank r-1's carry (the previous gather's record r-1); the other ranks send
		// their status word with it
		const uint64_t *carry = nullptr;
		for(uint32_t phase = 1;phase <= 2;++phase){
			for(uint32_t r = 0;r < W;++r){
				partial(r == me ? nv : 0u, r == me ? carry : nullptr, phase);
				gather();
				carry = ctx->sh_full.p + (size_t)r*stride + 1;
			}
		}
		r_lo = W - 1; r_hi = W;
	}
	if(rc_comm != PCR_OK) return rc_comm;
	hipLaunchKernelGGL(k_cov_combine, dim3(std::max(1u, (nv + 127)/128)), dim3(128), 0, ctx->stream, ctx->sh_full.p, stride, r_lo, r_hi, W, nv,
		ctx->opt_cov.p, ctx->sh_rec.p + stride);
	HIP_TRY(hipGetLastError());
	uint64_t st = 0;
	HIP_TRY(hipMemcpyAsync(cov_out.data(), ctx->opt_cov.p, (size_t)nv*sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
	HIP_TRY(hipMemcpyAsync(&st, ctx->sh_rec.p + stride, sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
	HIP_TRY(hipStreamSynchronize(ctx->stream));
	return sh_status_rc(st, local_rc, "pcr_optimize_batch");
}

// the fingerprint of an optimiser call: what it was asked, the arguments and the pool
uint64_t opt_fingerprint(uint64_t kind, const pcr_pair *assays, uint32_t n, const pcr_optimize_args *o, const pcr_pair *pool, uint32_t n_pool)
{
	uint64_t h = sh_hash(SH_HASH0, &kind, sizeof(kind));
	h = sh_hash(h, &n, sizeof(n));
	if(n) h = sh_hash(h, assays, (size_t)n*sizeof(pcr_pair));
	static_assert(sizeof(pcr_optimize_args) == offsetof(pcr_optimize_args, moves) + 8*sizeof(int32_t), "no padding to hash");
	h = sh_hash(h, o, offsetof(pcr_optimize_args, moves));
	h = sh_hash(h, o->moves, (size_t)std::max(0, std::min(8, o->n_moves))*sizeof(int32_t));
	h = sh_hash(h, &n_pool, sizeof(n_pool));
	if(n_pool) h = sh_hash(h, pool, (size_t)n_pool*sizeof(pcr_pair));
	return h;
}

// DRAIN + hipSetDevice as a status (the sharded entry points report it to the other ranks instead of returning on their own)
int enter_device(pcr_ctx *ctx)
{
	DRAIN(ctx);
	HIP_TRY(hipSetDevice(ctx->device));
	return PCR_OK;
}

// The weights' side of the exactness rule (DESIGN.md section 7), per rank: the smallest exponent q of a lowest set bit of a nonzero
// weight (every weight is an integer multiple of 2^q), the largest |w|, and whether any weight is not finite.
struct AttachRec { uint64_t status, first, n, n_total, want, nonfinite; int64_t q; double maxabs; };

void weight_facts(const std::vector<float> &w, AttachRec &a)
{
	a.q = INT64_MAX; a.maxabs = 0.0; a.nonfinite = 0;
	for(float x : w){
		if(!std::isfinite(x)){ a.nonfinite = 1; continue; }
		if(x == 0.0f) continue;
		const double m = std::fabs((double)x);
		a.maxabs = std::max(a.maxabs, m);
		int e = 0;
		const double f = std::frexp(m, &e);                                           // m = f * 2^e, f in [0.5, 1): 24 significant bits at most
		const uint64_t mi = (uint64_t)std::ldexp(f, 53);
		a.q = std::min<int64_t>(a.q, (int64_t)e - 53 + __builtin_ctzll(mi));
	}
}

// ---- pcr_shard_gather_bits: rank-local bitsets at arbitrary row boundaries -> bitsets over all n_total rows
// The record of a rank: [0] status word, [1 + v*pad + k] word k of its bitset v (pad = the largest local word count; words past
// its own count and every word of a rank that failed are zero).
__global__ void k_shard_pack(const uint64_t *__restrict__ local, uint64_t local_stride, uint64_t local_words, uint32_t n_vec, uint64_t pad,
	uint64_t status, uint64_t *__restrict__ rec)
{
	const uint64_t i = (uint64_t)blockIdx.x*blockDim.x + threadIdx.x;
	if(i == 0) rec[0] = status;
	if(i >= (uint64_t)n_vec*pad) return;
	const uint64_t v = i/pad, k = i - v*pad;
	rec[1 + i] = (local && k < local_words) ? local[v*local_stride + k] : 0ull;
}

// One thread per global output word (consecutive threads: consecutive words of one bitset, so the loads of a rank's words are
// contiguous too).  bounds[r] = rank r's first row, bounds[world] = n_total.  For every rank whose rows meet the word: the 64
// local bits that land in it (a funnel shift of two adjacent local words), masked to the part of the word the rank owns.
// Words at or past n_total are zero.  Thread 0 also ORs the status words into *status_out.
__global__ void k_shard_stitch(const uint64_t *__restrict__ full, uint64_t rec_words, uint64_t pad, const uint64_t *__restrict__ bounds,
	uint32_t world, uint32_t n_vec, uint64_t global_stride, uint64_t *__restrict__ global, uint64_t *__restrict__ status_out)
{
	const uint64_t i = (uint64_t)blockIdx.x*blockDim.x + threadIdx.x;
	if(i == 0){
		uint64_t st = 0;
		for(uint32_t r = 0;r < world;++r) st |= full[(size_t)r*rec_words];
		*status_out = st;
	}
	if(i >= (uint64_t)n_vec*global_stride) return;
	const uint64_t v = i/global_stride, gw = i - v*global_stride;
	const uint64_t base = gw*64, n_total = bounds[world];
	uint64_t out = 0;
	for(uint32_t r = 0;r < world && base < n_total;++r){
		const uint64_t f = bounds[r], e = min(bounds[r + 1], n_total);
		if(f >= e || e <= base || f >= base + 64) continue;
		const uint64_t *L = full + (size_t)r*rec_words + 1 + v*pad;
		const uint64_t nw = (e - f + 63)/64;
		uint64_t x;
		if(base >= f){
			const uint64_t off = base - f, lo = off >> 6;
			const uint32_t sh = (uint32_t)(off & 63);
			x = (lo < nw) ? (L[lo] >> sh) : 0ull;
			if(sh && lo + 1 < nw) x |= L[lo + 1] << (64 - sh);
		}
		else x = L[0] << (uint32_t)(f - base);                                      // 1 <= f - base <= 63
		const uint32_t lo_b = (uint32_t)(f > base ? f - base : 0), hi_b = (uint32_t)min<uint64_t>(64, e - base);
		const uint32_t width = hi_b - lo_b;
		const uint64_t m = (width == 64) ? ~0ull : (((1ull << width) - 1ull) << lo_b);
		out |= x & m;
	}
	global[v*global_stride + gw] = out;
}

// The gather itself (the ranks have agreed on n_vec): d_local = this rank's bitsets (nullptr or local_rc != PCR_OK: it sends
// zeros with its failure in the status word), d_global = the result (may be nullptr when local_rc != PCR_OK).  Returns the same
// code on every rank.
int shard_gather_bits_impl(pcr_ctx *ctx, const uint64_t *d_local, uint32_t n_vec, uint64_t local_stride, uint64_t *d_global,
	uint64_t global_stride, int local_rc)
{
	pcr_comm *c = ctx->shard_comm;
	const std::vector<uint64_t> &b = ctx->shard_bounds;
	const uint32_t W = (uint32_t)c->world;
	uint64_t pad = 0;
	for(uint32_t r = 0;r < W;++r) pad = std::max<uint64_t>(pad, (b[r + 1] - b[r] + 63)/64);
	const uint64_t rec_words = 1 + (uint64_t)n_vec*pad;
	int rc;
	if((rc = ctx->sh_rec.ensure((size_t)rec_words + 1)) != PCR_OK) return rc;
	if((rc = ctx->sh_full.ensure((size_t)rec_words*W)) != PCR_OK) return rc;
	const uint64_t me_words = (b[c->rank + 1] - b[c->rank] + 63)/64;
	const bool ok = local_rc == PCR_OK;
	const uint64_t n_pack = (uint64_t)n_vec*pad;
	hipLaunchKernelGGL(k_shard_pack, dim3((unsigned)std::max<uint64_t>(1, (n_pack + 255)/256)), dim3(256), 0, ctx->stream, ok ? d_local : nullptr,
		local_stride, me_words, n_vec, pad, ok ? 0ull : sh_fail_bit(local_rc), ctx->sh_rec.p);
	HIP_TRY(hipGetLastError());
	if((rc = sh_allgather_rec(ctx, c, ctx->sh_rec.p, rec_words, ctx->sh_full.p)) != PCR_OK) return rc;
	const uint32_t nv_out = (ok && d_global) ? n_vec : 0u;
	const uint64_t n_out = (uint64_t)nv_out*global_stride;
	hipLaunchKernelGGL(k_shard_stitch, dim3((unsigned)std::max<uint64_t>(1, (n_out + 255)/256)), dim3(256), 0, ctx->stream, ctx->sh_full.p, rec_words, pad,
		ctx->d_shard_bounds.p, W, nv_out, global_stride, d_global, ctx->sh_rec.p + rec_words);
	HIP_TRY(hipGetLastError());
	uint64_t st = 0;
	HIP_TRY(hipMemcpyAsync(&st, ctx->sh_rec.p + rec_words, sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
	HIP_TRY(hipStreamSynchronize(ctx->stream));
	return sh_status_rc(st, local_rc, "pcr_shard_gather_bits");
}

// a row's bytes as the sampler reads them: the length, then the packed bytes (the pad nibble of an odd length masked)
uint64_t sh_row_hash(uint64_t h, const uint8_t *bytes, uint64_t len)
{
	h = sh_hash(h, &len, sizeof(len));
	const uint64_t nb = (len + 1)/2;
	if(nb > 1) h = sh_hash(h, bytes, (size_t)nb - 1);
	if(nb){ const uint8_t last = (len & 1) ? (uint8_t)(bytes[nb - 1] & 0xF0) : bytes[nb - 1]; h = sh_hash(h, &last, 1); }
	return h;
}

} // namespace

extern "C" {

int pcr_shard_targets(pcr_ctx *ctx, pcr_comm *comm, uint64_t first_seq, uint64_t n_total)
{
	if(!ctx){ g_err = "pcr_shard_targets: bad argument"; return PCR_ERR_ARG; }
	if(!comm){ ctx->drop_shard(); return PCR_OK; }
	if(ctx->trial_comm){ g_err = "pcr_shard_targets: trial ranks are attached (pcr_design_trial_ranks); the two modes do not combine"; return PCR_ERR_STATE; }
	if(!comm->host_fn && comm->device != ctx->device){ g_err = "pcr_shard_targets: the communicator belongs to another device"; return PCR_ERR_ARG; }
	ctx->drop_shard();
	const SeqSet &S = ctx->sets[PCR_SET_TARGET];
	AttachRec me;
	memset(&me, 0, sizeof(me));
	int local_rc = enter_device(ctx);
	me.first = first_seq; me.n = S.n; me.n_total = n_total;
	weight_facts(S.weight, me);
	const char *env = getenv("PCRAMP_SHARD_COMBINE");
	const std::string want = env ? env : "auto";
	if(want == "chain") me.want = 2;
	else if(want == "exact" || want == "auto") me.want = 1;
	else if(local_rc == PCR_OK){ g_err = "pcr_shard_targets: PCRAMP_SHARD_COMBINE is not auto, exact or chain"; local_rc = PCR_ERR_ARG; }
	if(local_rc == PCR_OK && (first_seq > n_total || S.n > n_total - first_seq)){ g_err = "pcr_shard_targets: the shard lies outside [0, n_total)"; local_rc = PCR_ERR_ARG; }
	me.status = local_rc != PCR_OK ? sh_fail_bit(local_rc) : 0ull;
	std::vector<AttachRec> all((size_t)comm->world);
	ctx->shard_comm = comm;                                                        // (the RCCL staging buffer belongs to the handle)
	int rc = sh_allgather_host(ctx, comm, &me, sizeof(me), all.data());
	ctx->shard_comm = nullptr;
	if(rc != PCR_OK) return rc;
	uint64_t st = 0, next = 0;
	bool contiguous = true, nonfinite = false;
	int64_t q = INT64_MAX; double maxabs = 0.0; uint64_t want_mode = 1;
	for(const AttachRec &a : all){
		st |= a.status;
		contiguous = contiguous && a.first == next && a.n_total == n_total;
		next = a.first + a.n;
		nonfinite = nonfinite || a.nonfinite;
		q = std::min(q, a.q); maxabs = std::max(maxabs, a.maxabs); want_mode = std::max(want_mode, a.want);
	}
	if(st) return sh_status_rc(st, local_rc, "pcr_shard_targets");
	if(!contiguous || next != n_total){ g_err = "pcr_shard_targets: the ranks' ranges are not contiguous in rank order or do not cover n_total"; return PCR_ERR_ARG; }
	// exact partials: every weight is a multiple of 2^q and every partial sum is at most n_total * max|w| in magnitude; below
	// 2^52 * 2^q (one bit of margin for the rounding of the product) it is an integer multiple of 2^q with at most 52 bits: exact
	const bool exact = !nonfinite && (maxabs == 0.0 || (double)n_total*maxabs <= std::ldexp(1.0, (int)std::max<int64_t>(-1074, 52 + q)));
	ctx->shard_bounds.resize(all.size() + 1);
	for(size_t r = 0;r < all.size();++r) ctx->shard_bounds[r] = all[r].first;
	ctx->shard_bounds[all.size()] = n_total;
	if((rc = ctx->d_shard_bounds.ensure(ctx->shard_bounds.size())) != PCR_OK){ ctx->shard_bounds.clear(); return rc; }
	HIP_TRY(hipMemcpy(ctx->d_shard_bounds.p, ctx->shard_bounds.data(), ctx->shard_bounds.size()*sizeof(uint64_t), hipMemcpyHostToDevice));
	ctx->shard_comm = comm; ctx->shard_first = first_seq; ctx->shard_n_total = n_total;
	ctx->shard_mode = (want_mode == 1 && exact) ? 1 : 2;
	return PCR_OK;
}

int pcr_shard_gather_bits(pcr_ctx *ctx, const uint64_t *d_local, uint32_t n_vec, uint64_t local_stride_words, uint64_t *d_global,
	uint64_t global_stride_words)
{
	if(!ctx){ g_err = "pcr_shard_gather_bits: bad argument"; return PCR_ERR_ARG; }
	if(!ctx->shard_comm){ g_err = "pcr_shard_gather_bits: no target shard is attached (pcr_shard_targets)"; return PCR_ERR_STATE; }
	int local_rc = enter_device(ctx);
	const uint64_t n_me = ctx->sets[PCR_SET_TARGET].n;
	if(local_rc == PCR_OK && n_vec && (!d_local || !d_global || local_stride_words < (n_me + 63)/64 || global_stride_words < (ctx->shard_n_total + 63)/64)){
		g_err = "pcr_shard_gather_bits: bad argument (null buffer or a stride below the bitset's word count)"; local_rc = PCR_ERR_ARG;
	}
	// the record size depends on n_vec: the ranks agree on it first
	const int rc = shard_agree(ctx, sh_hash(SH_HASH0, &n_vec, sizeof(n_vec)), local_rc, "pcr_shard_gather_bits");
	if(rc != PCR_OK) return rc;
	if(n_vec == 0) return PCR_OK;
	return shard_gather_bits_impl(ctx, d_local, n_vec, local_stride_words, d_global, global_stride_words, PCR_OK);
}

int pcr_shard_sampler_targets(pcr_ctx *ctx, const uint8_t *packed4, const uint64_t *byte_offsets, const uint64_t *lengths, uint64_t n)
{
	if(!ctx){ g_err = "pcr_shard_sampler_targets: bad argument"; return PCR_ERR_ARG; }
	pcr_comm *c = ctx->shard_comm;
	if(!c){ g_err = "pcr_shard_sampler_targets: no target shard is attached (pcr_shard_targets)"; return PCR_ERR_STATE; }
	ctx->design_ready = false; ctx->samp_packed.clear(); ctx->samp_len.clear();
	const uint32_t W = (uint32_t)c->world;
	const std::vector<uint64_t> &b = ctx->shard_bounds;
	int local_rc = enter_device(ctx);
	// this rank's record: status, the n it was given, the hash of its own rows, and (rank 0) the hashes of its copy's slices
	std::vector<uint64_t> me(3 + W, 0);
	std::vector<std::vector<uint8_t> > copy;
	std::vector<uint64_t> copy_len;
	if(local_rc == PCR_OK){
		if(c->rank == 0 && (n != ctx->shard_n_total || (n && (!packed4 || !byte_offsets || !lengths)))){
			g_err = "pcr_shard_sampler_targets: rank 0 must pass the whole target set (n == n_total)"; local_rc = PCR_ERR_ARG;
		}
		else if(c->rank != 0 && (n != 0 || packed4 || byte_offsets || lengths)){
			g_err = "pcr_shard_sampler_targets: only rank 0 passes the target set (n = 0 and null pointers elsewhere)"; local_rc = PCR_ERR_ARG;
		}
	}
	if(local_rc == PCR_OK && c->rank == 0){
		copy.resize((size_t)n); copy_len.assign(lengths, lengths + n);
		for(uint64_t i = 0;i < n;++i) copy[i].assign(packed4 + byte_offsets[i], packed4 + byte_offsets[i] + (lengths[i] + 1)/2);
		for(uint32_t r = 0;r < W;++r){
			uint64_t h = SH_HASH0;
			for(uint64_t i = b[r];i < b[r + 1];++i) h = sh_row_hash(h, copy[i].data(), copy_len[i]);
			me[3 + r] = h;
		}
	}
	if(local_rc == PCR_OK){
		const SeqSet &T = ctx->sets[PCR_SET_TARGET];
		uint64_t h = SH_HASH0;
		for(uint32_t i = 0;i < T.n;++i) h = sh_row_hash(h, T.packed[i].data(), T.len[i]);
		me[1] = n; me[2] = h;
	}
	me[0] = local_rc != PCR_OK ? sh_fail_bit(local_rc) : 0ull;
	std::vector<uint64_t> all(me.size()*W);
	const int rc = sh_allgather_host(ctx, c, me.data(), me.size()*sizeof(uint64_t), all.data());
	if(rc != PCR_OK) return rc;
	uint64_t st = 0;
	for(uint32_t r = 0;r < W;++r) st |= all[(size_t)r*me.size()];
	if(st) return sh_status_rc(st, local_rc, "pcr_shard_sampler_targets");
	for(uint32_t r = 0;r < W;++r){
		if(all[3 + r] != all[(size_t)r*me.size() + 2]){
			g_err = "pcr_shard_sampler_targets: rank 0's copy differs from the rows of rank " + std::to_string(r); return PCR_ERR_ARG;
		}
	}
	ctx->samp_packed.swap(copy); ctx->samp_len.swap(copy_len);
	ctx->design_ready = true;
	return PCR_OK;
}

int pcr_shard_combine_mode(pcr_ctx *ctx) { return (ctx && ctx->shard_comm) ? ctx->shard_mode : 0; }

} // extern "C"
