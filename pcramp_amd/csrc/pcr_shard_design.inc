// The exchanges of the design loop over a target shard (pcr_design.inc; included just before it).  Besides the local search's
// own (pcr_shard.inc), the loop needs: every rank's weights and active flags once per call, rank 0's trials once per iteration,
// the unique amplicons of a trial over all targets at the record highs of the walk (the pool cover, pcr_multiplex_screen step
// (c)) and those of the best assay, and the best assay's target bits (shard_gather_bits_impl).  Every record starts with a
// status word, so a rank that failed locally still takes part and every rank returns the same code.

namespace {

// pcr_collect_amplicons into a vector that grows to what was found
int collect_amps(pcr_ctx *ctx, const pcr_pair *pair, float thr, int32_t amp_min, int32_t amp_max, std::vector<pcr_amplicon> &amp)
{
	amp.resize(4096);
	int64_t n = pcr_collect_amplicons(ctx, PCR_SET_TARGET, pair, thr, amp_min, amp_max, amp.data(), amp.size());
	if(n < 0) return (int)n;
	if((uint64_t)n > amp.size()){
		amp.resize((size_t)n);
		n = pcr_collect_amplicons(ctx, PCR_SET_TARGET, pair, thr, amp_min, amp_max, amp.data(), amp.size());
		if(n < 0) return (int)n;
	}
	amp.resize((size_t)n);
	return PCR_OK;
}

// the inner stretch of an amplicon of a loaded sequence, one code per byte (sequence.h:223-228)
int amp_codes(const SeqSet &T, const pcr_amplicon &r, std::vector<uint8_t> &codes)
{
	if(r.sequence >= T.n || r.inner_start < 0 || r.inner_length < 0 || (uint64_t)r.inner_start + (uint64_t)r.inner_length > T.len[r.sequence]){
		g_err = "pcr_design: amplicon outside its sequence"; return PCR_ERR_RANGE;
	}
	const std::vector<uint8_t> &buf = T.packed[r.sequence];
	codes.resize((size_t)r.inner_length);
	for(int32_t j = 0;j < r.inner_length;++j){
		const uint64_t p = (uint64_t)r.inner_start + (uint64_t)j;
		const uint8_t v = buf[(size_t)(p >> 1)];
		codes[(size_t)j] = (p & 1) ? (uint8_t)(v & 0xF) : (uint8_t)(v >> 4);
	}
	return PCR_OK;
}

// pcr_multiplex_screen step (c) after the collection: the pool assays against groups of unique amplicon stretches (group k =
// amp[first[k] .. first[k + 1])), one alignment pass over all of them; cover[k] = how many stretches of group k any pool assay hits
int pool_cover_pass(pcr_ctx *ctx, const std::vector<std::vector<uint8_t> > &amp, const std::vector<uint32_t> &first, const pcr_pair *pool,
	uint32_t n_pool, const pcr_multiplex_screen_args *a, float *cover)
{
	std::vector<uint8_t> packed; std::vector<uint64_t> off(amp.size()), len(amp.size());
	for(size_t i = 0;i < amp.size();++i){
		off[i] = packed.size(); len[i] = amp[i].size();
		for(size_t j = 0;j < amp[i].size();j += 2) packed.push_back((uint8_t)((amp[i][j] << 4) | ((j + 1 < amp[i].size()) ? amp[i][j + 1] : 0)));
	}
	int rc;
	if((rc = load_sequences_impl(ctx, PCR_SET_SCRATCH, packed.data(), off.data(), len.data(), nullptr, (uint32_t)amp.size())) != PCR_OK) return rc;
	const uint64_t words = (amp.size() + 63)/64;
	std::vector<uint64_t> bits((size_t)n_pool*words);
	if((rc = multiplex_match_impl(ctx, PCR_SET_SCRATCH, pool, n_pool, a->background_threshold, a->use_taq_mama, bits.data())) != PCR_OK) return rc;
	for(size_t k = 0;k + 1 < first.size();++k){
		// union over the pool (every pool assay sets bits in the same BitSet, main.cpp:792-797); amplicon Sequences carry the
		// default weight 1 (sequence.h:146), so weighted_coverage is the count -- a float sum of ones, exact
		double cov = 0.0;
		for(uint32_t s = first[k];s < first[k + 1];++s){
			bool hit = false;
			for(uint32_t i = 0;i < n_pool && !hit;++i) hit = ((bits[(size_t)i*words + s/64] >> (s % 64)) & 1u) != 0;
			if(hit) cov += 1.0;
		}
		cover[k] = (float)cov;
	}
	return PCR_OK;
}

// One status-and-size all-gather, then one all-gather of records padded to the largest: every rank's `words` u64 -> all of
// them, rank order, in `out` (first[r] .. first[r + 1] for rank r), over `c` (nullptr: the attached shard's communicator).
// Returns the same code on every rank.
int sh_gather_var(pcr_ctx *ctx, int local_rc, const std::vector<uint64_t> &words, std::vector<uint64_t> &out, std::vector<size_t> &first,
	pcr_comm *c = nullptr)
{
	if(!c) c = ctx->shard_comm;
	const size_t W = (size_t)c->world;
	const uint64_t me[2] = {local_rc != PCR_OK ? sh_fail_bit(local_rc) : 0ull, local_rc != PCR_OK ? 0ull : (uint64_t)words.size()};
	std::vector<uint64_t> hdr(2*W);
	int rc = sh_allgather_host(ctx, c, me, sizeof(me), hdr.data());
	if(rc != PCR_OK) return rc;
	uint64_t st = 0, pad = 0;
	for(size_t r = 0;r < W;++r){ st |= hdr[2*r]; pad = std::max(pad, hdr[2*r + 1]); }
	if(st) return sh_status_rc(st, local_rc, "pcr_design");
	out.clear(); first.assign(W + 1, 0);
	if(pad == 0) return PCR_OK;
	std::vector<uint64_t> send((size_t)pad, 0), recv((size_t)pad*W);
	std::copy(words.begin(), words.end(), send.begin());
	if((rc = sh_allgather_host(ctx, c, send.data(), pad*sizeof(uint64_t), recv.data())) != PCR_OK) return rc;
	for(size_t r = 0;r < W;++r){
		first[r] = out.size();
		out.insert(out.end(), recv.begin() + r*pad, recv.begin() + r*pad + hdr[2*r + 1]);
	}
	first[W] = out.size();
	return PCR_OK;
}

// The amplicons of `pair` over ALL targets: every rank collects over its rows (local_rc != PCR_OK: it sends nothing but its
// status), extracts their inner stretches, and the records (sequence made global) and stretches of all ranks come back in rank
// order.  Record: the pcr_amplicon (3 u64), then the stretch 8 codes per u64.
static_assert(sizeof(pcr_amplicon) == 24, "an amplicon record is 3 u64");
int shard_gather_amplicons(pcr_ctx *ctx, const pcr_pair *pair, const pcr_multiplex_screen_args *a, int local_rc, std::vector<pcr_amplicon> &amp_all,
	std::vector<std::vector<uint8_t> > &codes_all)
{
	const SeqSet &T = ctx->sets[PCR_SET_TARGET];
	std::vector<uint64_t> words;
	if(local_rc == PCR_OK){
		std::vector<pcr_amplicon> amp;
		local_rc = collect_amps(ctx, pair, a->target_threshold, a->amp_min, a->amp_max, amp);
		std::vector<uint8_t> codes;
		for(size_t i = 0;i < amp.size() && local_rc == PCR_OK;++i){
			if((local_rc = amp_codes(T, amp[i], codes)) != PCR_OK) break;
			pcr_amplicon g = amp[i];
			g.sequence = (uint32_t)(ctx->shard_first + g.sequence);
			const size_t at = words.size();
			words.resize(at + 3 + (codes.size() + 7)/8, 0);
			memcpy(&words[at], &g, sizeof(g));
			if(!codes.empty()) memcpy(&words[at + 3], codes.data(), codes.size());
		}
		if(local_rc != PCR_OK) words.clear();
	}
	std::vector<uint64_t> all; std::vector<size_t> first;
	const int rc = sh_gather_var(ctx, local_rc, words, all, first);
	if(rc != PCR_OK) return rc;
	amp_all.clear(); codes_all.clear();
	for(size_t at = 0;at < all.size();){
		pcr_amplicon g;
		memcpy(&g, &all[at], sizeof(g));
		if(g.inner_length < 0 || at + 3 + ((size_t)g.inner_length + 7)/8 > all.size()){ g_err = "pcr_design: a malformed amplicon record from a rank"; return PCR_ERR_STATE; }
		const uint8_t *p = (const uint8_t *)&all[at + 3];
		amp_all.push_back(g);
		codes_all.emplace_back(p, p + g.inner_length);
		at += 3 + ((size_t)g.inner_length + 7)/8;
	}
	return PCR_OK;
}

// pcr_multiplex_screen step (c) for one trial over all targets: the sort + unique of the union of the ranks' stretches is that
// of the whole set, so the cover is exact
int shard_pool_cover(pcr_ctx *ctx, const pcr_pair *pair, const pcr_pair *pool, uint32_t n_pool, const pcr_multiplex_screen_args *a, float &cover)
{
	std::vector<pcr_amplicon> amp; std::vector<std::vector<uint8_t> > codes;
	int rc = shard_gather_amplicons(ctx, pair, a, PCR_OK, amp, codes);
	if(rc != PCR_OK) return rc;
	std::sort(codes.begin(), codes.end());                                       // pcr_assay.cpp:805-806
	codes.erase(std::unique(codes.begin(), codes.end()), codes.end());
	cover = 0.0f;
	if(codes.empty()) return PCR_OK;
	const std::vector<uint32_t> first = {0u, (uint32_t)codes.size()};
	return pool_cover_pass(ctx, codes, first, pool, n_pool, a, &cover);
}

// every rank's weights and active flags -> the global vectors, in global index order
int shard_gather_rows(pcr_ctx *ctx, int local_rc, std::vector<float> &weight, std::vector<uint8_t> &active)
{
	const SeqSet &T = ctx->sets[PCR_SET_TARGET];
	const std::vector<uint64_t> &b = ctx->shard_bounds;
	const size_t W = (size_t)ctx->shard_comm->world;
	uint64_t pad = 0;
	for(size_t r = 0;r < W;++r) pad = std::max<uint64_t>(pad, b[r + 1] - b[r]);
	std::vector<uint64_t> me((size_t)pad + 1, 0), all(((size_t)pad + 1)*W);
	me[0] = local_rc != PCR_OK ? sh_fail_bit(local_rc) : 0ull;
	for(uint32_t i = 0;i < T.n && i < pad;++i){
		uint32_t wb; memcpy(&wb, &T.weight[i], 4);
		me[1 + i] = (uint64_t)wb | ((uint64_t)(T.active[i] ? 1u : 0u) << 32);
	}
	const int rc = sh_allgather_host(ctx, ctx->shard_comm, me.data(), me.size()*sizeof(uint64_t), all.data());
	if(rc != PCR_OK) return rc;
	uint64_t st = 0;
	for(size_t r = 0;r < W;++r) st |= all[r*(pad + 1)];
	if(st) return sh_status_rc(st, local_rc, "pcr_design");
	weight.assign((size_t)b[W], 0.0f); active.assign((size_t)b[W], 0);
	for(size_t r = 0;r < W;++r){
		for(uint64_t i = b[r];i < b[r + 1];++i){
			const uint64_t x = all[r*(pad + 1) + 1 + (i - b[r])];
			const uint32_t wb = (uint32_t)x;
			memcpy(&weight[(size_t)i], &wb, 4);
			active[(size_t)i] = (uint8_t)((x >> 32) & 1u);
		}
	}
	return PCR_OK;
}

// rank 0's trials to every rank: one all-gather of [status, the pairs] (the other ranks send their status and zeros)
static_assert(sizeof(pcr_pair) == 4*sizeof(uint64_t), "a pair is 4 u64");
int shard_share_trials(pcr_ctx *ctx, int local_rc, std::vector<pcr_pair> &trial)
{
	pcr_comm *c = ctx->shard_comm;
	const size_t rec = 1 + 4*trial.size(), W = (size_t)c->world;
	std::vector<uint64_t> me(rec, 0), all(rec*W);
	me[0] = local_rc != PCR_OK ? sh_fail_bit(local_rc) : 0ull;
	if(c->rank == 0 && local_rc == PCR_OK && !trial.empty()) memcpy(&me[1], trial.data(), trial.size()*sizeof(pcr_pair));
	const int rc = sh_allgather_host(ctx, c, me.data(), rec*sizeof(uint64_t), all.data());
	if(rc != PCR_OK) return rc;
	uint64_t st = 0;
	for(size_t r = 0;r < W;++r) st |= all[r*rec];
	if(st) return sh_status_rc(st, local_rc, "pcr_design");
	if(!trial.empty()) memcpy(trial.data(), &all[1], trial.size()*sizeof(pcr_pair));
	return PCR_OK;
}

// the fingerprint of a design call: the arguments, n_total, the command line and the output description's sizes
static_assert(sizeof(pcr_design_args) == 112, "no padding to hash");
uint64_t design_fingerprint(const pcr_design_args *a, uint64_t n_total, const pcr_output *o, int argc, const char *const *argv)
{
	uint64_t h = sh_hash(SH_HASH0, a, sizeof(*a));
	h = sh_hash(h, &n_total, sizeof(n_total));
	const uint64_t sizes[2] = {o->n_target, o->n_background};
	h = sh_hash(h, sizes, sizeof(sizes));
	h = sh_hash(h, &argc, sizeof(argc));
	for(int i = 0;i < argc;++i){
		const uint64_t n = argv[i] ? strlen(argv[i]) : ~0ull;
		h = sh_hash(h, &n, sizeof(n));
		if(argv[i]) h = sh_hash(h, argv[i], (size_t)n);
	}
	return h;
}

} // namespace
