// The design loop of the reference program (main.cpp:471-1130, one rank, one thread) over the entry points of this library
// (included by pcr_optimize.inc's tail): scope row f-7.  Nothing is computed here that does not have its own entry point and
// its own parity tests; what this call adds is the loop's bookkeeping -- the running rand_r seed, the order in which the trial
// assays meet the gates of main.cpp:737-866, the `best_score < s` comparisons, the assay ids, the active flags, the amplicon
// database of the multiplex background, the EOS splits -- and the output file, byte for byte (pcr_format_*).
//
// Where the reference walks the trial assays one by one, what EVERY trial needs is computed for the whole batch first (sampling,
// word DBs, the top-down start, the local search, the compatibility flags: each a pure function of the trial and of state that
// does not change inside an iteration); what only the record-setting trials need (the alignment-based covers) is asked for as the
// walk reaches them, as the reference does.
//
// Over a target shard (pcr_shard_targets + pcr_shard_sampler_targets) the same loop runs on every rank, with global host copies
// of the weights and active flags: rank 0 samples over its copy of the whole set and sends the trials; the target word DB,
// amplify and amplicon collection run over local rows; the pool cover and the best assay's amplicons and bits are gathered
// (pcr_shard_design.inc); the local search and the top-down start combine on their own.  Steps over data every rank holds
// whole (backgrounds, the multiplex set, the pool) compute the same on every rank; a failure in a step over local rows is kept
// in `lrc` and travels in the status word of the next exchange, so that every rank returns the same code.
//
// With trial ranks attached (pcr_design_trial_ranks, the reference's MPI mode) every rank holds the whole sets and runs the loop
// as one rank does, on its own trials from the seed `seed + rank`; after the walk the ranks' best assays are reduced to one
// winner (pcr_trial_ranks.inc), whose target bits and amplicons the winning rank sends; the rest of the iteration is the one-rank
// code on every rank.  Here too a local failure is kept in `lrc` and travels in the status word of the next exchange.

namespace {

struct DesignState { std::vector<pcr_pair> pool; };

// summed weights of the active sequences in index order, float accumulation (main.cpp:603, :649)
inline float active_norm(const std::vector<float> &weight, const std::vector<uint8_t> &active, uint32_t &n_active)
{
	float norm = 0.0f; n_active = 0;
	for(size_t i = 0;i < active.size();++i){ if(active[i]){ ++n_active; norm += weight[i]; } }
	return norm;
}

inline int append_text(std::string &text, int64_t (*fn)(char *, uint64_t, void *), void *arg)
{
	const int64_t need = fn(nullptr, 0, arg);
	if(need < 0) return (int)need;
	const size_t at = text.size();
	text.resize(at + (size_t)need + 1);
	const int64_t got = fn(&text[at], (uint64_t)need + 1, arg);
	if(got != need){ g_err = "pcr_design: a writer changed its mind about its length"; return PCR_ERR_STATE; }
	text.resize(at + (size_t)need);
	return PCR_OK;
}

// Trial ranks: the winner's target bits and amplicons, from the winning rank to every rank.  They depend on the word DB of the
// iteration, which only the winning rank built from its own trials (main.cpp:906-908), so they are computed there and shipped, as
// the reference ships them (:1421-1601).  The winning rank's record: its t_words bitset words, then per amplicon the pcr_amplicon
// (3 u64) and its inner stretch 8 codes per u64; every other rank sends nothing.  Returns the same code on every rank.
int trial_share_winner(pcr_ctx *ctx, size_t win, const pcr_pair *best, const pcr_amplify_args *find_args, bool use_multiplex,
	uint64_t t_words, std::vector<uint64_t> &target_match, std::vector<pcr_amplicon> &amp, std::vector<std::vector<uint8_t> > &codes_all)
{
	const SeqSet &T = ctx->sets[PCR_SET_TARGET];
	std::vector<uint64_t> words;
	int local_rc = PCR_OK;
	if((size_t)ctx->trial_comm->rank == win){
		words.assign((size_t)t_words, 0);
		local_rc = pcr_amplify(ctx, PCR_SET_TARGET, best, 1, find_args, words.data(), nullptr, nullptr, nullptr);
		std::vector<pcr_amplicon> mine;
		if(local_rc == PCR_OK && use_multiplex) local_rc = collect_amps(ctx, best, find_args->ident_threshold, find_args->amp_min, find_args->amp_max, mine);
		std::vector<uint8_t> codes;
		for(size_t i = 0;i < mine.size() && local_rc == PCR_OK;++i){
			if((local_rc = amp_codes(T, mine[i], codes)) != PCR_OK) break;
			const size_t at = words.size();
			words.resize(at + 3 + (codes.size() + 7)/8, 0);
			memcpy(&words[at], &mine[i], sizeof(pcr_amplicon));
			if(!codes.empty()) memcpy(&words[at + 3], codes.data(), codes.size());
		}
		if(local_rc != PCR_OK) words.clear();
	}
	std::vector<uint64_t> all; std::vector<size_t> first;
	const int rc = sh_gather_var(ctx, local_rc, words, all, first, ctx->trial_comm);
	if(rc != PCR_OK) return rc;
	const size_t lo = first[win], hi = first[win + 1];
	if(hi - lo < t_words){ g_err = "pcr_design: a malformed winner record"; return PCR_ERR_STATE; }
	target_match.assign(all.begin() + lo, all.begin() + lo + t_words);
	amp.clear(); codes_all.clear();
	for(size_t at = lo + t_words;at < hi;){
		pcr_amplicon g;
		if(at + 3 > hi){ g_err = "pcr_design: a malformed winner record"; return PCR_ERR_STATE; }
		memcpy(&g, &all[at], sizeof(g));
		if(g.inner_length < 0 || at + 3 + ((size_t)g.inner_length + 7)/8 > hi){ g_err = "pcr_design: a malformed winner record"; return PCR_ERR_STATE; }
		const uint8_t *p = (const uint8_t *)&all[at + 3];
		amp.push_back(g);
		codes_all.emplace_back(p, p + g.inner_length);
		at += 3 + ((size_t)g.inner_length + 7)/8;
	}
	return PCR_OK;
}

// PCR::total_degeneracy (assay.h:536-539)
inline double total_degeneracy(const pcr_pair &p)
{
	return pcrhost::planes_degeneracy(pcrhost::planes_of_word(p.f.w)) + pcrhost::planes_degeneracy(pcrhost::planes_of_word(p.r.w));
}

} // namespace

extern "C" {

int pcr_design(pcr_ctx *ctx, const pcr_design_args *a, const pcr_output *o, int argc, const char *const *argv,
	pcr_pair *pool_out, uint32_t pool_cap, uint32_t *n_pool_out)
{
	if(!ctx || !a || !o || argc < 0 || (argc && !argv) || (pool_cap && !pool_out)){ g_err = "pcr_design: bad argument"; return PCR_ERR_ARG; }
	if(ctx->shard_comm && !ctx->design_ready){ g_err = "pcr_design: a target shard is attached (pcr_shard_targets) but the handle is not design-ready (pcr_shard_sampler_targets)"; return PCR_ERR_STATE; }
	const bool sharded = ctx->shard_comm != nullptr;
	pcr_comm *const ranks = sharded ? nullptr : ctx->trial_comm;                              // the reference's MPI mode
	const bool ranked = ranks != nullptr, carry = sharded || ranked;                          // carry: a local failure waits for the next collective
	SeqSet &T = ctx->sets[PCR_SET_TARGET], &B = ctx->sets[PCR_SET_BACKGROUND];
	const uint64_t n_all = sharded ? ctx->shard_n_total : T.n;                                // the targets the loop designs over
	int lrc = PCR_OK;                                                                          // this rank's outcome since the last exchange
	if(n_all == 0){ g_err = "pcr_design: no target sequences loaded"; lrc = PCR_ERR_STATE; }
	else if(o->n_target != n_all || o->n_background != B.n){ g_err = "pcr_design: the output description does not match the loaded sets"; lrc = PCR_ERR_ARG; }
	else if(a->num_trial == 0 || a->num_trial > (1u << 20)){ g_err = "pcr_design: num_trial out of range"; lrc = PCR_ERR_ARG; }
	if(!carry && lrc != PCR_OK) return lrc;
	int rc;
	std::vector<float> g_weight; std::vector<uint8_t> g_active;                                // all n_all targets, global index order
	auto now_ms = [](){ return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
	double t_exchange = 0.0;
	if(sharded){
		const double t0 = now_ms();
		if(lrc == PCR_OK) lrc = enter_device(ctx);
		if((rc = shard_agree(ctx, lrc == PCR_OK ? design_fingerprint(a, n_all, o, argc, argv) : 0ull, lrc, "pcr_design")) != PCR_OK) return rc;
		if((rc = shard_gather_rows(ctx, PCR_OK, g_weight, g_active)) != PCR_OK) return rc;
		t_exchange += now_ms() - t0;
	}
	else if(ranked){
		// the same call on every rank, over the same sets as they stand now
		const double t0 = now_ms();
		if(lrc == PCR_OK) lrc = enter_device(ctx);
		uint64_t fp = 0;
		if(lrc == PCR_OK){ const uint64_t hs = trial_sets_hash(ctx); fp = design_fingerprint(a, n_all, o, argc, argv); fp = sh_hash(fp, &hs, sizeof(hs)); }
		if((rc = shard_agree(ctx, fp, lrc, "pcr_design", ranks)) != PCR_OK) return rc;
		g_weight = T.weight; g_active = T.active;
		t_exchange += now_ms() - t0;
	}
	else{
		DRAIN(ctx);
		HIP_TRY(hipSetDevice(ctx->device));
		g_weight = T.weight; g_active = T.active;
	}
	// pcr_set_active on this rank's slice of the global flags
	auto set_local_active = [&]() -> int {
		return pcr_set_active(ctx, PCR_SET_TARGET, g_active.data() + (sharded ? ctx->shard_first : 0));
	};
	DesignState D;
	ctx->design_text.clear();
	// ---- options as the entry points take them
	pcr_optimize_args oa; memset(&oa, 0, sizeof(oa));
	oa.max_degen = a->max_degen; oa.primer_min = a->primer_min; oa.primer_max = a->primer_max; oa.thermo = a->thermo;
	oa.target.collect_threshold = a->target_threshold*a->target_search_multiplier;            // float product, as assay.h:407
	oa.target.ident_threshold = a->target_threshold;
	oa.target.amp_min = a->target_amp_min; oa.target.amp_max = a->target_amp_max; oa.target.use_taq_mama = a->use_taq_mama;
	oa.background.collect_threshold = a->background_threshold*a->background_search_multiplier;
	oa.background.ident_threshold = a->background_threshold;
	oa.background.amp_min = a->background_amp_min; oa.background.amp_max = a->background_amp_max; oa.background.use_taq_mama = a->use_taq_mama;
	oa.have_background = B.n > 0; oa.use_multiplex = a->use_multiplex; oa.multiplex_threshold = a->background_threshold;
	oa.n_moves = 0;                                                                            // main.cpp:82-95
	if(a->max_degen > 1.0){ oa.moves[oa.n_moves++] = PCR_MOVE_INCREASE_DEGENERACY; oa.moves[oa.n_moves++] = PCR_MOVE_DECREASE_DEGENERACY; }
	if(a->optimize_5){ oa.moves[oa.n_moves++] = PCR_MOVE_TRIM5; oa.moves[oa.n_moves++] = PCR_MOVE_GROW5; }
	if(a->optimize_3){ oa.moves[oa.n_moves++] = PCR_MOVE_TRIM3; oa.moves[oa.n_moves++] = PCR_MOVE_GROW3; }
	const pcr_sampler_args sa = {a->primer_min, a->primer_max, a->target_amp_min, a->target_amp_max, a->max_degen};
	const uint32_t min_len = (uint32_t)std::max(0, a->primer_min);                             // Options::min_oligo_length(), pcramp.h:138-141
	const uint32_t min_len_bg = (uint32_t)((double)(int)min_len*0.9);                         // main.cpp:595: int * double -> const unsigned int &
	pcr_background_args ba; memset(&ba, 0, sizeof(ba));
	ba.collect_threshold = oa.background.collect_threshold; ba.background_threshold = a->background_threshold;
	ba.amp_min = a->background_amp_min; ba.amp_max = a->background_amp_max; ba.use_taq_mama = a->use_taq_mama; ba.evaluate_all_amplicons = 0;
	pcr_multiplex_screen_args ma; memset(&ma, 0, sizeof(ma));
	ma.thermo = a->thermo; ma.background_threshold = a->background_threshold; ma.use_taq_mama = a->use_taq_mama;
	ma.target_threshold = a->target_threshold; ma.amp_min = a->target_amp_min; ma.amp_max = a->target_amp_max;
	const pcr_amplify_args find_args = {a->target_threshold, a->target_threshold, a->target_amp_min, a->target_amp_max, a->use_taq_mama};   // pcr_assay.cpp:556

	struct Hdr { const pcr_output *o; int argc; const char *const *argv; uint32_t seed; };
	Hdr hdr = {o, argc, argv, a->seed};
	if((rc = append_text(ctx->design_text, [](char *out, uint64_t cap, void *p) -> int64_t { const Hdr *h = (const Hdr *)p; return pcr_format_header(h->o, h->argc, h->argv, h->seed, out, cap); }, &hdr)) != PCR_OK) return rc;

	uint32_t global_seed = a->seed + (ranked ? (uint32_t)ranks->rank : 0u);                  // main.cpp:99-113: every task's seed is seed + rank
	uint32_t assay_iteration = 0, major_id = 1, minor_id = 1;
	const uint64_t t_words = (T.n + 63)/64, g_words = (n_all + 63)/64, b_words = (B.n + 63)/64;
	std::vector<uint64_t> total_background(std::max<uint64_t>(b_words, 1), 0);
	std::vector<std::vector<uint8_t> > amplicon_codes;                                         // multiplex_background_seq, in the order it grew
	const uint32_t n_trial = a->num_trial;
	while(true){
		++assay_iteration;
		double t_mark = now_ms(), t_phase[8] = {t_exchange, 0, 0, 0, 0, 0, 0, 0};
		t_exchange = 0.0;
		auto lap = [&](int k){ const double t = now_ms(); t_phase[k] += t - t_mark; t_mark = t; };
		uint32_t targets_remaining = 0;
		for(uint8_t x : g_active) targets_remaining += x ? 1u : 0u;
		if(targets_remaining == 0){                                                             // main.cpp:488-502
			std::fill(g_active.begin(), g_active.end(), (uint8_t)1);
			rc = set_local_active();
			if(!carry && rc != PCR_OK) return rc;
			if(lrc == PCR_OK) lrc = rc;
			targets_remaining = (uint32_t)n_all; ++major_id; minor_id = 1;
		}
		struct It { const pcr_output *o; uint32_t it, major, minor, remaining; };
		It itr = {o, assay_iteration, major_id, minor_id, targets_remaining};
		if((rc = append_text(ctx->design_text, [](char *out, uint64_t cap, void *p) -> int64_t { const It *h = (const It *)p; return pcr_format_iteration(h->o, h->it, h->major, h->minor, h->remaining, out, cap); }, &itr)) != PCR_OK) return rc;
		// ---- this rank's walk: the trials, their local search and the gates; its best assay
		ScoreH best_score = EMPTY_SCORE;
		pcr_pair best_assay; memset(&best_assay, 0, sizeof(best_assay));
		std::vector<uint64_t> best_background(std::max<uint64_t>(b_words, 1), 0);
		uint32_t num_active_background = 0, num_active_target = 0;
		float active_background_norm = 0.0f, active_target_norm = 0.0f;
		auto walk = [&]() -> int {
		// ---- the trial assays (main.cpp:538-550, one thread: one local seed per iteration)
		uint32_t local_seed = pcr_host_rand_r(&global_seed);
		std::vector<pcr_pair> trial(n_trial);
		if(!sharded){ if((rc = pcr_random_assays(ctx, PCR_SET_TARGET, &local_seed, n_trial, &sa, &a->thermo, trial.data(), nullptr)) != PCR_OK) return rc; }
		else{
			// rank 0 samples over its copy of the whole set with the global flags; the trials go to every rank with its status
			if(ctx->shard_comm->rank == 0 && lrc == PCR_OK){
				const SampView v = {ctx->samp_packed.data(), ctx->samp_len.data(), g_active.data(), (uint32_t)n_all};
				lrc = sampler_args_ok(&sa) ? random_assays_view(ctx, v, &local_seed, n_trial, &sa, &a->thermo, trial.data(), nullptr) : PCR_ERR_ARG;
			}
			lap(0);
			if((rc = shard_share_trials(ctx, lrc, trial)) != PCR_OK) return rc;
			lap(7);
		}
		lap(0);
		// ---- the word DBs for them (main.cpp:579-615, :644-691)
		if(B.n > 0){
			active_background_norm = active_norm(B.weight, B.active, num_active_background);
			if((rc = pcr_select_words(ctx, PCR_SET_BACKGROUND, trial.data(), n_trial, a->optimize_5, a->optimize_3, oa.background.collect_threshold, min_len_bg, nullptr)) != PCR_OK) return rc;
		}
		active_target_norm = active_norm(g_weight, g_active, num_active_target);
		rc = pcr_select_words(ctx, PCR_SET_TARGET, trial.data(), n_trial, a->optimize_5, a->optimize_3, oa.target.collect_threshold, min_len, nullptr);
		if(!sharded && rc != PCR_OK) return rc;
		lap(1);
		if(sharded){                                                                            // (the local target DB's outcome)
			if((rc = shard_agree(ctx, 0ull, rc, "pcr_design")) != PCR_OK) return rc;
			lap(7);
		}
		// ---- top-down start and local search of every trial (main.cpp:707-735)
		std::vector<uint8_t> usable(n_trial, 1);
		if(a->top_down_search){ if((rc = pcr_make_degenerate(ctx, trial.data(), n_trial, &oa, usable.data())) != PCR_OK) return rc; }
		std::vector<uint32_t> idx;
		for(uint32_t t = 0;t < n_trial;++t){ if(usable[t]) idx.push_back(t); }
		std::vector<pcr_pair> cand(idx.size()), opt(idx.size());
		std::vector<float> sc(3*idx.size());
		for(size_t k = 0;k < idx.size();++k) cand[k] = trial[idx[k]];
		if(!idx.empty()){
			if((rc = pcr_optimize_batch(ctx, cand.data(), (uint32_t)cand.size(), &oa, D.pool.data(), (uint32_t)D.pool.size(), opt.data(), sc.data(), nullptr)) != PCR_OK) return rc;
		}
		lap(2);
		// the first gate (main.cpp:737-741): the approximate scores
		std::vector<uint32_t> gate;                                                             // indices into idx / opt
		for(size_t k = 0;k < idx.size();++k){
			if(sc[3*k + 1] > a->max_background_cover || sc[3*k] < a->min_target_cover) continue;
			gate.push_back((uint32_t)k);
		}
		std::vector<pcr_pair> gp(gate.size());
		for(size_t g = 0;g < gate.size();++g) gp[g] = opt[gate[g]];
		// PCR::multiplex_compatible of every gated trial with every pooled assay: one thermodynamics launch (detail = none: flags only)
		std::vector<uint8_t> compatible(gate.size(), 1);
		if(a->use_multiplex && !gate.empty() && !D.pool.empty()){
			std::vector<uint8_t> none(gate.size(), 0);
			std::vector<float> mc(gate.size()), pc(gate.size());
			if((rc = pcr_multiplex_screen(ctx, gp.data(), (uint32_t)gp.size(), D.pool.data(), (uint32_t)D.pool.size(), &ma, none.data(), compatible.data(), mc.data(), pc.data())) != PCR_OK) return rc;
		}
		// ---- the walk over the trials in their order (main.cpp:743-866).  The alignment-based covers are asked for only where the
		// reference computes them -- for a trial that beats the running best, i.e. at the record highs of the sequence of scores, a
		// handful per iteration -- one trial per call.
		std::vector<uint64_t> bits(std::max<uint64_t>(b_words, 1), 0);
		for(size_t g = 0;g < gate.size();++g){
			const size_t k = gate[g];
			ScoreH s = {sc[3*k], 0.0f, sc[3*k + 2]};                                             // "Recompute the background coverage" (:744)
			if(a->use_multiplex){
				if(!compatible[g]) continue;                                                      // :748-757
				if(score_lt(best_score, s)){
					uint8_t ok1 = 1; float mc1 = 0.0f, pc1 = 0.0f;
					if(!sharded){ if((rc = pcr_multiplex_screen(ctx, &gp[g], 1, D.pool.data(), (uint32_t)D.pool.size(), &ma, nullptr, &ok1, &mc1, &pc1)) != PCR_OK) return rc; }
					else{
						// (a) is `compatible`, (b) runs over the multiplex set every rank holds; (c) needs the amplicons over all targets
						if((rc = pcr_multiplex_screen(ctx, &gp[g], 1, nullptr, 0, &ma, nullptr, &ok1, &mc1, &pc1)) != PCR_OK) return rc;
						if(!D.pool.empty()){
							lap(3);
							if((rc = shard_pool_cover(ctx, &gp[g], D.pool.data(), (uint32_t)D.pool.size(), &ma, pc1)) != PCR_OK) return rc;
							lap(7);
						}
					}
					s.bc += mc1;                                                                   // :767-771
					if(s.bc <= a->max_background_cover) s.bc += pc1;                               // :783-803
				}
			}
			const double deg_best = total_degeneracy(best_assay), deg_trial = total_degeneracy(gp[g]);
			if(num_active_background > 0){
				if(score_lt(best_score, s) && s.bc <= a->max_background_cover){                    // :815-816
					if((rc = pcr_background_match(ctx, PCR_SET_BACKGROUND, &gp[g], 1, &ba, bits.data())) != PCR_OK) return rc;
					s.bc += pcr_weighted_coverage(bits.data(), B.weight.data(), B.n);               // :826
					const bool update_best = (s.bc <= a->max_background_cover) && (score_lt(best_score, s) || (score_eq(best_score, s) && deg_best > deg_trial));
					if(update_best){ best_score = s; best_assay = gp[g]; best_background = bits; }
				}
			}
			else{
				const bool update_best = (s.bc <= a->max_background_cover) && (score_lt(best_score, s) || (score_eq(best_score, s) && deg_best > deg_trial));   // :846-857
				if(update_best){ best_score = s; best_assay = gp[g]; }
			}
		}
		return PCR_OK;
		};
		if(!ranked){ if((rc = walk()) != PCR_OK) return rc; }
		else if(lrc == PCR_OK) lrc = walk();
		lap(3);
		size_t win = 0;                                                                         // trial ranks: the winning rank
		if(ranked){
			// reduce_best_assay (main.cpp:1421-1601), before the test below as the reference does (:926-932): rank 0's best is the
			// starting best; in ascending rank order a record replaces it iff it scores higher or ties with a lower degeneracy
			// (:1432-1480; the reference's root takes the ranks in arrival order, DESIGN.md section 5)
			const float mine[3] = {best_score.tc, best_score.bc, best_score.ov};
			std::vector<uint64_t> recs; std::vector<TrialBest> all;
			if((rc = trial_gather_best(ctx, lrc, mine, best_assay, best_background, b_words, recs, all)) != PCR_OK) return rc;
			for(size_t r = 1;r < all.size();++r){
				const ScoreH sw = {all[win].tc, all[win].bc, all[win].ov}, sr = {all[r].tc, all[r].bc, all[r].ov};
				if(score_lt(sw, sr) || (score_eq(sw, sr) && total_degeneracy(all[win].assay) > total_degeneracy(all[r].assay))) win = r;
			}
			if(ctx->debug_log){
				for(size_t r = 0;r < all.size();++r) fprintf(stderr, "[pcramp] design iteration %u, rank %zu of %d: best %g %g %g, degeneracy %g%s\n", assay_iteration, r,
					ranks->world, all[r].tc, all[r].bc, all[r].ov, total_degeneracy(all[r].assay), r == win ? " (the winner)" : "");
			}
			best_score = {all[win].tc, all[win].bc, all[win].ov};
			best_assay = all[win].assay;
			std::copy(all[win].background, all[win].background + b_words, best_background.begin());
			lap(7);
		}
		if(best_score.tc <= 0.0f) break;                                                        // :926-930: nothing detects a target
		auto apply = [&]() -> int {
		// ---- the best assay: the targets it detects, its amplicons (main.cpp:898-922)
		std::vector<uint64_t> target_match(t_words, 0);
		rc = ranked ? PCR_OK : pcr_amplify(ctx, PCR_SET_TARGET, &best_assay, 1, &find_args, target_match.data(), nullptr, nullptr, nullptr);
		if(!sharded && rc != PCR_OK) return rc;
		std::vector<pcr_amplicon> amp;
		std::vector<std::vector<uint8_t> > amp_codes_all;                                      // sharded, trial ranks: the inner stretches of `amp`
		if(ranked){
			// from the winning rank, whose word DB found them
			lap(4);
			if((rc = trial_share_winner(ctx, win, &best_assay, &find_args, a->use_multiplex != 0, t_words, target_match, amp, amp_codes_all)) != PCR_OK) return rc;
			lap(7);
		}
		else if(sharded){
			// the bits over all targets; then the amplicons over all targets, records with global sequence indices
			lrc = rc;
			lap(4);
			if(lrc == PCR_OK && (lrc = ctx->sh_bits.ensure((size_t)(t_words + g_words))) == PCR_OK){
				const hipError_t e = hipMemcpyAsync(ctx->sh_bits.p, target_match.data(), t_words*sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream);
				if(e != hipSuccess){ g_err = std::string("pcr_design: ") + hipGetErrorString(e); lrc = PCR_ERR_DEVICE; }
			}
			if((rc = shard_gather_bits_impl(ctx, ctx->sh_bits.p, 1u, t_words, lrc == PCR_OK ? ctx->sh_bits.p + t_words : nullptr, g_words, lrc)) != PCR_OK) return rc;
			target_match.assign(g_words, 0);
			HIP_TRY(hipMemcpyAsync(target_match.data(), ctx->sh_bits.p + t_words, g_words*sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
			HIP_TRY(hipStreamSynchronize(ctx->stream));
			if(a->use_multiplex){ if((rc = shard_gather_amplicons(ctx, &best_assay, &ma, PCR_OK, amp, amp_codes_all)) != PCR_OK) return rc; }
			lap(7);
		}
		else if(a->use_multiplex){
			amp.resize(4096);
			int64_t n = pcr_collect_amplicons(ctx, PCR_SET_TARGET, &best_assay, a->target_threshold, a->target_amp_min, a->target_amp_max, amp.data(), amp.size());
			if(n < 0) return (int)n;
			if((uint64_t)n > amp.size()){
				amp.resize((size_t)n);
				n = pcr_collect_amplicons(ctx, PCR_SET_TARGET, &best_assay, a->target_threshold, a->target_amp_min, a->target_amp_max, amp.data(), amp.size());
				if(n < 0) return (int)n;
			}
			amp.resize((size_t)n);
		}
		lap(4);
		// ---- the record (main.cpp:950-1103)
		pcr_assay_record rec; memset(&rec, 0, sizeof(rec));
		rec.major_id = major_id; rec.minor_id = minor_id; rec.assay = best_assay;
		rec.target_coverage = best_score.tc; rec.background_coverage = best_score.bc;
		rec.active_target_norm = active_target_norm; rec.active_background_norm = active_background_norm; rec.num_active_background = num_active_background;
		rec.target_match = target_match.data(); rec.background_match = B.n ? best_background.data() : nullptr;
		struct As { const pcr_output *o; const pcr_assay_record *rec; const pcr_pair *pool; uint32_t n_pool; };
		As as = {o, &rec, D.pool.data(), (uint32_t)D.pool.size()};
		if((rc = append_text(ctx->design_text, [](char *out, uint64_t cap, void *p) -> int64_t { const As *h = (const As *)p; return pcr_format_assay(h->o, h->rec, h->pool, h->n_pool, out, cap); }, &as)) != PCR_OK) return rc;
		// ---- the multiplex background grows by the assay's unique amplicons; the targets are split (main.cpp:989-1017)
		if(a->use_multiplex){
			std::vector<std::vector<uint8_t> > mine;
			if(sharded || ranked) mine.swap(amp_codes_all);
			else for(const pcr_amplicon &r : amp){
				if(r.sequence >= T.n || r.inner_start < 0 || r.inner_length < 0 || (uint64_t)r.inner_start + (uint64_t)r.inner_length > T.len[r.sequence]){ g_err = "pcr_design: amplicon outside its sequence"; return PCR_ERR_RANGE; }
				const std::vector<uint8_t> &buf = T.packed[r.sequence];
				std::vector<uint8_t> codes((size_t)r.inner_length);
				for(int32_t j = 0;j < r.inner_length;++j){
					const uint64_t p = (uint64_t)r.inner_start + (uint64_t)j;
					const uint8_t v = buf[(size_t)(p >> 1)];
					codes[(size_t)j] = (p & 1) ? (uint8_t)(v & 0xF) : (uint8_t)(v >> 4);         // sequence.h:223-228
				}
				mine.push_back(std::move(codes));
			}
			std::sort(mine.begin(), mine.end());                                                 // pcr_assay.cpp:805-806
			mine.erase(std::unique(mine.begin(), mine.end()), mine.end());
			for(std::vector<uint8_t> &c : mine) amplicon_codes.push_back(std::move(c));
			if(!amplicon_codes.empty()){
				std::vector<uint8_t> packed; std::vector<uint64_t> off(amplicon_codes.size()), len(amplicon_codes.size());
				for(size_t i = 0;i < amplicon_codes.size();++i){
					const std::vector<uint8_t> &c = amplicon_codes[i];
					off[i] = packed.size(); len[i] = c.size();
					for(size_t j = 0;j < c.size();j += 2) packed.push_back((uint8_t)((c[j] << 4) | ((j + 1 < c.size()) ? c[j + 1] : 0)));
				}
				if(packed.empty()) packed.push_back(0);
				if((rc = pcr_multiplex_load(ctx, packed.data(), off.data(), len.data(), (uint32_t)amplicon_codes.size(), min_len, nullptr)) != PCR_OK) return rc;
				if((rc = pcr_load_sequences(ctx, PCR_SET_MULTIPLEX, packed.data(), off.data(), len.data(), nullptr, (uint32_t)amplicon_codes.size())) != PCR_OK) return rc;
			}
			// (an amplicon whose last primer hangs over the end of its sequence -- a partial word matched there -- has `end` at or past
			// the sequence's length: the reference's split_sequence then writes past the logical end of its buffer, sequence.h:232-241,
			// which leaves the sequence as it was; here such a split is skipped.  A negative `begin` makes AmpliconBounds throw, assay.h:85.)
			// (sharded: `amp` holds every rank's amplicons with global indices; a rank splits its own rows, rank 0 its copy too)
			std::vector<uint32_t> sp_seq; std::vector<uint64_t> sp_pos;
			const bool copy = sharded && ctx->shard_comm->rank == 0;
			for(const pcr_amplicon &r : amp){
				if(r.begin < 0 || r.begin > r.end){ g_err = "AmpliconBounds(): Amplicon begin > amplicon end"; return PCR_ERR_RANGE; }
				const int64_t at[3] = {r.begin, (int64_t)(((uint32_t)r.begin + (uint32_t)r.end)/2u), r.end};
				const uint64_t first = sharded ? ctx->shard_first : 0;
				const bool mine_row = r.sequence >= first && r.sequence - first < T.n;
				for(int k = 0;k < 3;++k){
					if(copy && r.sequence < n_all && (uint64_t)at[k] < ctx->samp_len[r.sequence]){
						uint8_t &v = ctx->samp_packed[r.sequence][(size_t)((uint64_t)at[k] >> 1)];
						v = (at[k] & 1) ? (v & 0xF0) : (v & 0x0F);                                   // sequence.h:232-241
					}
					if(!mine_row || (uint64_t)at[k] >= T.len[r.sequence - first]) continue;
					sp_seq.push_back(r.sequence - (uint32_t)first); sp_pos.push_back((uint64_t)at[k]);
				}
			}
			rc = pcr_split_many(ctx, PCR_SET_TARGET, sp_seq.data(), sp_pos.data(), (uint32_t)sp_seq.size());
			if(!sharded && rc != PCR_OK) return rc;
			if(lrc == PCR_OK) lrc = rc;
		}
		lap(5);
		// ---- the detected targets leave the search; the assay joins the pool (main.cpp:1105-1124)
		for(uint64_t i = 0;i < n_all;++i){ if((target_match[i/64] >> (i % 64)) & 1u) g_active[(size_t)i] = 0; }
		if(lrc == PCR_OK){
			rc = set_local_active();
			if(!sharded && rc != PCR_OK) return rc;
			lrc = rc;
		}
		for(uint64_t w = 0;w < b_words;++w) total_background[w] |= best_background[w];
		D.pool.push_back(best_assay);
		lap(6);
		return PCR_OK;
		};
		if(!ranked){ if((rc = apply()) != PCR_OK) return rc; }
		else lrc = apply();                                                                     // (lrc was PCR_OK: the reduction agreed)
		if(ctx->timing) fprintf(stderr, "[pcramp] design iteration %u ms: sample %.1f  word DBs %.1f  local search %.1f  gates %.1f  best assay %.1f  amplicon DB + splits %.1f  flags %.1f  %s %.1f\n",
			assay_iteration, t_phase[0], t_phase[1], t_phase[2], t_phase[3], t_phase[4], t_phase[5], t_phase[6], ranked ? "reduction" : "exchanges", t_phase[7]);
		if(assay_iteration >= a->num_assay) break;
	}
	if(carry){ if((rc = shard_agree(ctx, 0ull, lrc, "pcr_design", ranks)) != PCR_OK) return rc; }   // (the last iteration's splits and flags)
	{
		struct Ft { const pcr_output *o; const uint8_t *act; const uint64_t *bg; };
		Ft ft = {o, g_active.data(), B.n ? total_background.data() : nullptr};
		if((rc = append_text(ctx->design_text, [](char *out, uint64_t cap, void *p) -> int64_t { const Ft *h = (const Ft *)p; return pcr_format_footer(h->o, h->act, h->bg, out, cap); }, &ft)) != PCR_OK) return rc;
	}
	if(n_pool_out) *n_pool_out = (uint32_t)D.pool.size();
	for(size_t i = 0;i < D.pool.size() && i < pool_cap;++i) pool_out[i] = D.pool[i];
	return PCR_OK;
}

const char *pcr_design_output(pcr_ctx *ctx, uint64_t *len_out)
{
	if(!ctx){ if(len_out) *len_out = 0; return nullptr; }
	if(len_out) *len_out = ctx->design_text.size();
	return ctx->design_text.c_str();
}

} // extern "C"
