// The reference's own MPI mode (main.cpp:60-113, :344, :434, :926-927, :1420-1601) behind pcr_design: every rank holds the
// whole target and background sets, samples its own trials from `seed + rank`, runs the unchanged local walk over them, and
// the ranks' best assays are reduced to one winner that every rank then applies (include/pcramp_hip.h:
// pcr_design_trial_ranks).  Included after pcr_shard.inc, whose status words, hashes and all-gathers it uses; the design loop
// (pcr_design.inc) calls the steps below.
//
// The reduction is ONE all-gather of a fixed-size record per rank per iteration: the status word, the rank's best Score, its
// best assay and its background bits.  The winner's target bits and amplicons follow from the winning rank alone
// (pcr_design.inc: trial_share_winner): they come from the iteration's word DB, which that rank built from its own trials.

namespace {

// An FNV-style multiply-xor over 8-byte words, the tail bytewise (sh_hash): a C2 target set, 50 MB packed, in milliseconds
inline uint64_t tr_hash(uint64_t h, const void *p, size_t bytes)
{
	const uint8_t *b = (const uint8_t *)p;
	size_t i = 0;
	for(;i + 8 <= bytes;i += 8){ uint64_t w; memcpy(&w, b + i, 8); h ^= w; h *= 0x100000001B3ull; h ^= h >> 29; }
	return sh_hash(h, b + i, bytes - i);
}

// A hash of the state of one sequence set as the design loop reads it: count, lengths, the packed bytes (EOS splits applied; the
// pad nibble of an odd length is zero since the load), weights and active flags.  Equal on every rank iff the ranks would design
// over the same set.
uint64_t trial_set_hash(const SeqSet &S)
{
	uint64_t h = SH_HASH0;
	const uint64_t n = S.n;
	h = sh_hash(h, &n, sizeof(n));
	for(uint32_t i = 0;i < S.n;++i){
		h = sh_hash(h, &S.len[i], sizeof(uint64_t));
		h = tr_hash(h, S.packed[i].data(), S.packed[i].size());
	}
	if(S.n){
		h = tr_hash(h, S.weight.data(), S.weight.size()*sizeof(float));
		h = tr_hash(h, S.active.data(), S.active.size());
	}
	return h;
}

uint64_t trial_sets_hash(const pcr_ctx *ctx)
{
	const uint64_t ht = trial_set_hash(ctx->sets[PCR_SET_TARGET]), hb = trial_set_hash(ctx->sets[PCR_SET_BACKGROUND]);
	return sh_hash(ht, &hb, sizeof(hb));
}

// The reduction record of a rank: [0] status, [1] target and background coverage (float bits), [2] oligo overlap, [3, 7) the best
// assay, [7, 7 + b_words) its background bits.  A rank that failed sends its status and zeros.
constexpr uint64_t TR_HEAD = 7;
static_assert(sizeof(pcr_pair) == 4*sizeof(uint64_t), "a pair is 4 u64");

struct TrialBest { float tc, bc, ov; pcr_pair assay; const uint64_t *background; };

// Every rank's best of the iteration -> `all` (world records of TR_HEAD + b_words u64, rank order) and the views of them in
// `best`.  Returns the same code on every rank: any rank's failure (local_rc) is carried in its status word.
int trial_gather_best(pcr_ctx *ctx, int local_rc, const float score[3], const pcr_pair &assay, const std::vector<uint64_t> &background,
	uint64_t b_words, std::vector<uint64_t> &all, std::vector<TrialBest> &best)
{
	pcr_comm *c = ctx->trial_comm;
	const size_t W = (size_t)c->world, rec = (size_t)(TR_HEAD + b_words);
	std::vector<uint64_t> me(rec, 0);
	me[0] = local_rc != PCR_OK ? sh_fail_bit(local_rc) : 0ull;
	if(local_rc == PCR_OK){
		uint32_t f[3];
		memcpy(f, score, sizeof(f));
		me[1] = (uint64_t)f[0] | ((uint64_t)f[1] << 32);
		me[2] = (uint64_t)f[2];
		memcpy(&me[3], &assay, sizeof(pcr_pair));
		for(uint64_t w = 0;w < b_words && w < background.size();++w) me[TR_HEAD + w] = background[w];
	}
	all.assign(rec*W, 0);
	const int rc = sh_allgather_host(ctx, c, me.data(), rec*sizeof(uint64_t), all.data());
	if(rc != PCR_OK) return rc;
	uint64_t st = 0;
	for(size_t r = 0;r < W;++r) st |= all[r*rec];
	if(st) return sh_status_rc(st, local_rc, "pcr_design");
	best.resize(W);
	for(size_t r = 0;r < W;++r){
		const uint64_t *p = &all[r*rec];
		const uint32_t f[3] = {(uint32_t)p[1], (uint32_t)(p[1] >> 32), (uint32_t)p[2]};
		memcpy(&best[r].tc, &f[0], 4); memcpy(&best[r].bc, &f[1], 4); memcpy(&best[r].ov, &f[2], 4);
		memcpy(&best[r].assay, &p[3], sizeof(pcr_pair));
		best[r].background = p + TR_HEAD;
	}
	return PCR_OK;
}

} // namespace

extern "C" {

int pcr_design_trial_ranks(pcr_ctx *ctx, pcr_comm *comm)
{
	if(!ctx){ g_err = "pcr_design_trial_ranks: bad argument"; return PCR_ERR_ARG; }
	if(!comm){ ctx->trial_comm = nullptr; return PCR_OK; }
	if(ctx->shard_comm){ g_err = "pcr_design_trial_ranks: a target shard is attached (pcr_shard_targets); the two modes do not combine"; return PCR_ERR_STATE; }
	if(!comm->host_fn && comm->device != ctx->device){ g_err = "pcr_design_trial_ranks: the communicator belongs to another device"; return PCR_ERR_ARG; }
	ctx->trial_comm = nullptr;
	const int local_rc = enter_device(ctx);
	// status, then per set: count and the state hash
	const SeqSet &T = ctx->sets[PCR_SET_TARGET], &B = ctx->sets[PCR_SET_BACKGROUND];
	const uint64_t me[5] = {local_rc != PCR_OK ? sh_fail_bit(local_rc) : 0ull, (uint64_t)T.n, trial_set_hash(T), (uint64_t)B.n, trial_set_hash(B)};
	std::vector<uint64_t> all(5*(size_t)comm->world);
	const int rc = sh_allgather_host(ctx, comm, me, sizeof(me), all.data());
	if(rc != PCR_OK) return rc;
	uint64_t st = 0; bool same = true;
	for(int r = 0;r < comm->world;++r){
		st |= all[5*(size_t)r];
		for(int k = 1;k < 5;++k) same = same && all[5*(size_t)r + k] == me[k];
	}
	if(st) return sh_status_rc(st, local_rc, "pcr_design_trial_ranks");
	if(!same){ g_err = "pcr_design_trial_ranks: the ranks' target or background sets differ"; return PCR_ERR_ARG; }
	ctx->trial_comm = comm;
	return PCR_OK;
}

int pcr_design_trial_world(pcr_ctx *ctx) { return (ctx && ctx->trial_comm) ? ctx->trial_comm->world : 0; }

} // extern "C"
