// The multiplex compatibility filter of the trial loop (main.cpp:744-803), batched over the trial assays (included by
// pcr_device.hip).  Nothing new is computed here: the three quantities are PCR::multiplex_compatible (pcr_assay.cpp:815-852),
// find_multiplex_background_match (background_match.cpp:168-295) and collect_unique_amplicons (pcr_assay.cpp:756-813), each
// of which has its own entry point and its own parity tests; this call runs them for ALL trial assays with one
// thermodynamics launch, one alignment pass over the multiplex set and one over all trials' amplicons.  The amplicons
// themselves are still collected with one pcr_collect_amplicons call per asked-for trial (step (c): a launch and a host wait
// each -- the filter is asked for the handful of trials that survive the earlier gates of main.cpp:737-778, via `detail`; a
// caller that asks for all 1 000 pays 1 000 small launches: batching that collection by trial is the open item here).

extern "C" {

int pcr_multiplex_screen(pcr_ctx *ctx, const pcr_pair *trial, uint32_t n_trial, const pcr_pair *pool, uint32_t n_pool,
	const pcr_multiplex_screen_args *a, const uint8_t *detail, uint8_t *compatible, float *multiplex_cover, float *pool_cover)
{
	if(!ctx || !a || (n_trial && (!trial || !compatible || !multiplex_cover || !pool_cover)) || (n_pool && !pool)){
		g_err = "pcr_multiplex_screen: bad argument"; return PCR_ERR_ARG;
	}
	DRAIN(ctx);
	HIP_TRY(hipSetDevice(ctx->device));
	for(uint32_t t = 0;t < n_trial;++t){ compatible[t] = 1; multiplex_cover[t] = 0.0f; pool_cover[t] = 0.0f; }
	if(n_trial == 0) return PCR_OK;
	int rc;
	// ---- (a) every pool assay against every trial assay (main.cpp:748-752; the pool assay is `this`)
	if(n_pool){
		std::vector<pcr_pair> pa((size_t)n_trial*n_pool), pb((size_t)n_trial*n_pool);
		for(uint32_t t = 0;t < n_trial;++t) for(uint32_t i = 0;i < n_pool;++i){ pa[(size_t)t*n_pool + i] = pool[i]; pb[(size_t)t*n_pool + i] = trial[t]; }
		std::vector<uint8_t> ok(pa.size());
		if((rc = pcr_multiplex_compatible(ctx, pa.data(), pb.data(), (uint32_t)pa.size(), &a->thermo, ok.data())) != PCR_OK) return rc;
		for(uint32_t t = 0;t < n_trial;++t) for(uint32_t i = 0;i < n_pool;++i){ if(!ok[(size_t)t*n_pool + i]) compatible[t] = 0; }
	}
	std::vector<uint32_t> want;                                                   // the trials whose covers are asked for
	for(uint32_t t = 0;t < n_trial;++t){ if(compatible[t] && (!detail || detail[t])) want.push_back(t); }
	if(want.empty()) return PCR_OK;
	// ---- (b) the trial assays against the amplicons accepted so far (main.cpp:767-771)
	SeqSet &M = ctx->sets[PCR_SET_MULTIPLEX];
	if(M.n){
		std::vector<pcr_pair> wp(want.size());
		for(size_t k = 0;k < want.size();++k) wp[k] = trial[want[k]];
		const uint64_t words = (M.n + 63)/64;
		std::vector<uint64_t> bits(wp.size()*words);
		if((rc = multiplex_match_impl(ctx, PCR_SET_MULTIPLEX, wp.data(), (uint32_t)wp.size(), a->background_threshold, a->use_taq_mama, bits.data())) != PCR_OK) return rc;
		for(size_t k = 0;k < want.size();++k) multiplex_cover[want[k]] = pcr_weighted_coverage(bits.data() + k*words, M.weight.data(), M.n);
	}
	if(n_pool == 0) return PCR_OK;
	// ---- (c) the pool assays against every trial's own amplicons (main.cpp:786-803): the unique amplicon stretches of all
	// asked-for trials become the sequences of the scratch set, one alignment pass serves them all
	SeqSet &T = ctx->sets[PCR_SET_TARGET];
	std::vector<std::vector<uint8_t> > amp;                                       // codes, one byte per base
	std::vector<uint32_t> first(want.size() + 1, 0);
	std::vector<pcr_amplicon> rec(4096);
	for(size_t k = 0;k < want.size();++k){
		first[k] = (uint32_t)amp.size();
		int64_t n = pcr_collect_amplicons(ctx, PCR_SET_TARGET, &trial[want[k]], a->target_threshold, a->amp_min, a->amp_max, rec.data(), rec.size());
		if(n < 0) return (int)n;
		if((uint64_t)n > rec.size()){
			rec.resize((size_t)n);
			n = pcr_collect_amplicons(ctx, PCR_SET_TARGET, &trial[want[k]], a->target_threshold, a->amp_min, a->amp_max, rec.data(), rec.size());
			if(n < 0) return (int)n;
		}
		std::vector<std::vector<uint8_t> > mine;
		for(int64_t i = 0;i < n;++i){
			const pcr_amplicon &r = rec[(size_t)i];
			if(r.sequence >= T.n || (uint64_t)r.inner_start + r.inner_length > T.len[r.sequence]){ g_err = "pcr_multiplex_screen: amplicon outside its sequence"; return PCR_ERR_RANGE; }
			const std::vector<uint8_t> &buf = T.packed[r.sequence];
			std::vector<uint8_t> codes(r.inner_length);
			for(uint32_t j = 0;j < r.inner_length;++j){
				const uint64_t p = (uint64_t)r.inner_start + j;
				const uint8_t v = buf[(size_t)(p >> 1)];
				codes[j] = (p & 1) ? (uint8_t)(v & 0xF) : (uint8_t)(v >> 4);             // sequence.h:223-228
			}
			mine.push_back(std::move(codes));
		}
		std::sort(mine.begin(), mine.end());                                       // identical amplicons come from different targets (pcr_assay.cpp:805-806)
		mine.erase(std::unique(mine.begin(), mine.end()), mine.end());
		for(std::vector<uint8_t> &c : mine) amp.push_back(std::move(c));
	}
	first[want.size()] = (uint32_t)amp.size();
	if(amp.empty()) return PCR_OK;
	std::vector<float> cover(want.size());
	if((rc = pool_cover_pass(ctx, amp, first, pool, n_pool, a, cover.data())) != PCR_OK) return rc;
	for(size_t k = 0;k < want.size();++k) pool_cover[want[k]] = cover[k];
	return PCR_OK;
}

} // extern "C"
