// Random assay sampler (scope row f-2): PCR::random_assay (pcr_assay.cpp:580-734) driven by glibc's
// rand_r, reproduced draw for draw so that a whole run samples the assays the reference samples at
// --thread 1 (main.cpp:538-550).
//
// The walk over the random stream is sequential -- which draws an attempt consumes depends on which
// filter rejects it -- but everything an attempt can need from the device is a function of the stream
// position it starts at (and of the target sequence already picked).  So the host speculates: for every
// start position p of a window of the stream it derives the attempt that WOULD start there (lengths,
// forward start, forward oligo; reverse start and reverse oligo as they would be drawn if the forward
// oligo passes), puts the thermodynamic jobs of all of them (is_valid of F, is_valid of R, F x R
// heterodimer) into ONE k_thermo_wave launch, and then walks the stream over the finished results.  The same
// launch carries the next few trials as they would start if each one before succeeds at its first attempt.
// Included by pcr_entry_sw_thermo.inc.

namespace {

struct SpecAttempt {
	int early;                     // > 0: rejected before any thermodynamics after this many draws
	const char *throws_f;          // the reference throws while building F (reached as soon as the attempt starts)
	const char *throws_r;          // ... while building R (reached only when F is valid)
	bool r_checks;                 // amplicon length, EOS, degeneracy and split tests of the R half pass
	Planes F, R;
	int f_start, amp_len;
	uint32_t fj0, fj1, rj0, rj1, dj0, dj1;   // job ranges
};

inline int sampler_nibble(const std::vector<uint8_t> &buf, int64_t i)             // sequence.h:223-228
{
	const uint8_t v = buf[(size_t)(i >> 1)];
	return (i & 1) ? (v & 0xF) : (v >> 4);
}

// Sequence::subword (sequence.cpp:269-302) into slots 0.. ; Word::push_back drops EOS nibbles
// (word.cpp:31-48), so fewer than `len` occupied slots means the stretch crosses a record boundary.
inline int sampler_subword(const std::vector<uint8_t> &buf, int64_t loc, int len, uint64_t w[2])
{
	w[0] = w[1] = 0;
	int n = 0;
	for(int i = 0;i < len;++i){
		const unsigned v = (unsigned)sampler_nibble(buf, loc + i);
		if(v) pcrhost::word_set(w, n++, v);
	}
	return n;
}

inline Planes planes_center(Planes p)                                            // word.h:392-418
{
	const int left = pcrhost::planes_start(p);
	int right = pcrhost::planes_stop(p);
	if(left > right) return p;
	right = 32 - right;
	const int delta = (right - left)/2;
	for(int i = 0;i < delta;++i) p = pcrhost::planes_shift_right(p);
	for(int i = 0;i > delta;--i) p = pcrhost::planes_shift_left(p);
	return p;
}

inline bool jobs_valid(const std::vector<thermo::JobOut> &res, uint32_t j0, uint32_t j1, const pcr_thermo_args *a)
{
	for(uint32_t k = j0;k < j1;++k){
		const thermo::JobOut &o = res[k];
		if(o.tm_pm < a->tm_min || o.tm_pm > a->tm_max) return false;              // valid_pcr.cpp:19-23
		if(o.tm_hairpin > a->max_hairpin) return false;                          // :27-31
		if(o.tm_dimer > a->max_dimer) return false;                              // :34-41 (check_homo_dimer = true)
	}
	return true;
}

// The attempt that starts at stream position p (rv[p..p+3] are its draws) on a target of `len` bases.
bool speculate(const std::vector<uint8_t> &buf, int len, const int *rv, const pcr_sampler_args *o, const pcr_thermo_args *th,
	SpecAttempt &a, std::vector<thermo::Job> &jobs)
{
	memset(&a, 0, sizeof(a));
	const int span = o->primer_max - o->primer_min + 1;
	const int f_len = o->primer_min + rv[0] % span;                               // pcr_assay.cpp:637-638
	const int r_len = o->primer_min + rv[1] % span;
	if(f_len + r_len > len){ a.early = 2; return true; }                         // :640
	const int f_start = rv[2] % ((len + 1) - o->amp_min);                         // :644, sample.cpp:12
	a.f_start = f_start;
	if((int64_t)f_start + f_len > len){ a.throws_f = "Sequence::subword: word is out of bounds"; return true; }
	uint64_t w[2];
	if(sampler_subword(buf, f_start, f_len, w) != f_len){ a.early = 3; return true; }   // :649
	a.F = pcrhost::planes_of_word(w);
	if(pcrhost::planes_degeneracy(a.F) > o->max_degen){ a.early = 3; return true; }     // :655
	a.fj0 = (uint32_t)jobs.size();
	if(!append_valid_jobs(a.F, th, 1, jobs)) return false;
	a.fj1 = (uint32_t)jobs.size();
	// the R half, as drawn when F passes (:677-715)
	const int lo = f_start + o->amp_min - r_len;
	const int hi = std::min((len + 1) - r_len, (f_start + o->amp_max + 1) - r_len);
	const int r_start = lo + rv[3] % (hi - lo);                                   // hi - lo >= 1 whenever len >= amp_min <= amp_max
	const int amp_len = r_start - f_start + r_len;
	a.amp_len = amp_len;
	if(amp_len > o->amp_max || amp_len < o->amp_min) return true;                // :683-686
	if(r_start < 0 || (int64_t)r_start + r_len > len){ a.throws_r = "Sequence::subword: word is out of bounds"; return true; }
	if(sampler_subword(buf, r_start, r_len, w) != r_len) return true;            // :693
	a.R = pcrhost::planes_revcomp(pcrhost::planes_of_word(w));                    // :688
	for(int k = pcrhost::planes_start(a.R);k > 0;--k) a.R = pcrhost::planes_shift_left(a.R);   // Word::complement() fills from slot 0 (word.h:140-183); center() rounds from there
	if(pcrhost::planes_degeneracy(a.R) > o->max_degen) return true;              // :697
	for(int i = 0;i < amp_len;++i){ if(sampler_nibble(buf, (int64_t)f_start + i) == 0) return true; }   // has_split, :703
	a.r_checks = true;
	a.rj0 = (uint32_t)jobs.size();
	if(!append_valid_jobs(a.R, th, 1, jobs)) return false;
	a.rj1 = a.dj0 = (uint32_t)jobs.size();
	if(!append_dimer_jobs(a.F, a.R, th, jobs)) return false;
	a.dj1 = (uint32_t)jobs.size();
	return true;
}

// A window of the random stream on one target: the attempts that could start at its first `window` positions.
struct SpecWindow {
	uint32_t seed_before_pick = 0;   // stream state at which this trial's target pick is drawn (chain windows)
	uint32_t si = 0;
	int window = 0;
	std::vector<int> rv;
	std::vector<uint32_t> state;     // state[p] = stream state before draw p (p = 0: right after the pick)
	std::vector<SpecAttempt> spec;
};

// What the sampler reads of a sequence set: the packed bytes (as loaded, splits applied), lengths and active flags of n sequences --
// a loaded SeqSet, or the host-only copy of the whole target set that rank 0 of a sharded design loop samples from.
struct SampView { const std::vector<uint8_t> *packed; const uint64_t *len; const uint8_t *active; uint32_t n; };

bool build_window(const SampView &S, uint32_t si, uint32_t s0, int window, const pcr_sampler_args *o, const pcr_thermo_args *th,
	SpecWindow &w, std::vector<thermo::Job> &jobs)
{
	w.si = si; w.window = window;
	w.rv.resize(window + 3); w.state.resize(window + 4);
	uint32_t s = s0;
	for(int p = 0;p < window + 3;++p){ w.state[p] = s; w.rv[p] = (int)pcrhost::rand_r_glibc(&s); }
	w.state[window + 3] = s;
	w.spec.resize(window);
	const int len = (int)S.len[si];
	for(int p = 0;p < window;++p){ if(!speculate(S.packed[si], len, w.rv.data() + p, o, th, w.spec[p], jobs)) return false; }
	return true;
}

// The reference's attempt loop (pcr_assay.cpp:626-734) over a finished window.  1: assay found (`hit`), 0: the
// window or the budget of 100 attempts ran out, < 0: the reference throws here.  p_end = draws consumed.
int walk_window(const SpecWindow &w, const std::vector<thermo::JobOut> &res, const pcr_thermo_args *th, unsigned &attempts,
	const SpecAttempt *&hit, int &p_end)
{
	int p = 0;
	while(p < w.window && attempts < 100){
		const SpecAttempt &a = w.spec[p];
		++attempts;
		if(a.early){ p += a.early; continue; }
		if(a.throws_f){ g_err = a.throws_f; return PCR_ERR_RANGE; }
		if(!jobs_valid(res, a.fj0, a.fj1, th)){ p += 3; continue; }               // :662
		p += 4;
		if(a.throws_r){ g_err = a.throws_r; return PCR_ERR_RANGE; }
		if(!a.r_checks) continue;
		if(!jobs_valid(res, a.rj0, a.rj1, th)) continue;                          // :710
		float m = 0.0f;
		for(uint32_t k = a.dj0;k < a.dj1;++k) m = std::max(m, res[k].tm_dimer);   // pcr_assay.cpp:262
		if(m > th->max_dimer) continue;                                           // :715
		hit = &a; p_end = p;
		return 1;
	}
	p_end = p;                                                                    // <= window + 3
	return 0;
}

bool sampler_args_ok(const pcr_sampler_args *o)
{
	if(o->primer_min < 1 || o->primer_max < o->primer_min || o->primer_max > 32 || o->amp_min < 1 || o->amp_max < o->amp_min){
		g_err = "pcr_random_assays: bad primer or amplicon range"; return false;
	}
	return true;
}

// pcr_random_assays over a view (the arguments are checked by the caller)
int random_assays_view(pcr_ctx *ctx, const SampView &S, uint32_t *seed, uint32_t n_trials, const pcr_sampler_args *o,
	const pcr_thermo_args *th, pcr_pair *pairs_out, pcr_sample_info *info_out)
{
	std::vector<uint32_t> act;                                                   // pcr_assay.cpp:593-599
	for(uint32_t i = 0;i < S.n;++i){ if(S.active[i]) act.push_back(i); }
	if(act.empty()){ g_err = "PCR::random_assay: No active sequences found"; return PCR_ERR_ARG; }
	// Most trials succeed at their first or second attempt, so a launch for one trial is mostly round trip.  A launch
	// therefore carries a CHAIN of trials: trial k+1 is speculated from the state trial k leaves if its first attempt
	// succeeds (pick + 4 draws); the chain is used as far as the walk confirms it and rebuilt from the real state
	// otherwise.  A trial that outlives its first window (rare) continues alone with wider windows.
	const int FIRST_WINDOW = 16, NEXT_WINDOW = 192;     // stream positions per window
	const uint32_t CHAIN = 6;
	std::vector<SpecWindow> chain;
	size_t ci = 0;
	SpecWindow alone;
	std::vector<thermo::Job> jobs;
	std::vector<thermo::JobOut> chain_res, alone_res;
	for(uint32_t t = 0;t < n_trials;++t){
		if(ci >= chain.size() || chain[ci].seed_before_pick != *seed){
			chain.clear(); ci = 0; jobs.clear();
			uint32_t s = *seed;
			const uint32_t want = std::min<uint32_t>(CHAIN, n_trials - t);
			for(uint32_t k = 0;k < want;++k){
				chain.emplace_back();
				SpecWindow &w = chain.back();
				w.seed_before_pick = s;
				uint32_t sp = s;
				const uint32_t sk = act[pcrhost::rand_r_glibc(&sp) % act.size()];       // :618
				if((int)S.len[sk] < o->amp_min){                                     // :622-624 -- only if the walk really gets here
					chain.pop_back();
					if(k == 0){ g_err = "PCR::random_assay: sequence length is too small!"; return PCR_ERR_ARG; }
					break;
				}
				if(!build_window(S, sk, sp, FIRST_WINDOW, o, th, w, jobs)){ g_err = "pcr_random_assays: oligo cannot be expanded"; return PCR_ERR_CAPACITY; }
				s = w.state[4];
			}
			const int rc = run_thermo_jobs(ctx, jobs, th->salt, chain_res);
			if(rc != PCR_OK) return rc;
		}
		unsigned seq_iter = 1, attempts = 0;
		const SpecAttempt *hit = nullptr;
		int p_end = 0;
		uint32_t si;
		bool done;
		{
			const SpecWindow &w = chain[ci++];
			si = w.si;
			const int r = walk_window(w, chain_res, th, attempts, hit, p_end);
			if(r < 0) return r;
			*seed = w.state[p_end];
			done = (r == 1);
		}
		while(!done){
			if(attempts >= 100){                                                     // :626-634: another sequence
				if(++seq_iter > 100){ g_err = "PCR::random_assay: Unable to generate a valid initial assay to test!"; return PCR_ERR_RANGE; }   // :611-613
				si = act[pcrhost::rand_r_glibc(seed) % act.size()];                  // :618
				if((int)S.len[si] < o->amp_min){ g_err = "PCR::random_assay: sequence length is too small!"; return PCR_ERR_ARG; }
				attempts = 0;
			}
			jobs.clear();
			if(!build_window(S, si, *seed, NEXT_WINDOW, o, th, alone, jobs)){ g_err = "pcr_random_assays: oligo cannot be expanded"; return PCR_ERR_CAPACITY; }
			const int rc = run_thermo_jobs(ctx, jobs, th->salt, alone_res);
			if(rc != PCR_OK) return rc;
			const int r = walk_window(alone, alone_res, th, attempts, hit, p_end);
			if(r < 0) return r;
			*seed = alone.state[p_end];
			done = (r == 1);
		}
		pcrhost::word_of_planes(planes_center(hit->F), pairs_out[t].f.w);              // :719
		pcrhost::word_of_planes(planes_center(hit->R), pairs_out[t].r.w);
		if(info_out){
			pcr_sample_info &I = info_out[t];
			I.sequence = si; I.f_start = hit->f_start; I.amplicon_length = hit->amp_len;
			I.sequence_iterations = seq_iter; I.assay_iterations = attempts;
		}
	}
	return PCR_OK;
}

} // namespace

extern "C" {

uint32_t pcr_host_rand_r(uint32_t *seed) { return pcrhost::rand_r_glibc(seed); }

int pcr_random_assays(pcr_ctx *ctx, pcr_set which, uint32_t *seed, uint32_t n_trials, const pcr_sampler_args *o,
	const pcr_thermo_args *th, pcr_pair *pairs_out, pcr_sample_info *info_out)
{
	if(!set_ok(which)){ g_err = "pcr_random_assays: unknown sequence set"; return PCR_ERR_ARG; }
	if(!ctx || !seed || !o || !th || (which != PCR_SET_TARGET && which != PCR_SET_BACKGROUND) || (n_trials && !pairs_out)){
		g_err = "pcr_random_assays: bad argument"; return PCR_ERR_ARG;
	}
	if(!sampler_args_ok(o)) return PCR_ERR_ARG;
	FLUSH(ctx);
	HIP_TRY(hipSetDevice(ctx->device));
	const SeqSet &S = ctx->sets[which];
	const SampView v = {S.packed.data(), S.len.data(), S.active.data(), S.n};
	return random_assays_view(ctx, v, seed, n_trials, o, th, pairs_out, info_out);
}

} // extern "C"
