// make_degenerate (optimize.cpp:356-398 -> PCR::maximize_degeneracy, pcr_assay.cpp:111-230): the opt-in top-down start of the local
// search (--optimize.top-down, main.cpp:709-721), for a batch of trial assays.  Included at the end of pcr_optimize.inc.
//
// The reference, per assay: collect_target_candidates + update_target_candidates (the candidate amplicons and the identity of F / R
// with their keys), sort the amplicons by sqrtf(f identity x r identity), descending (std::sort, assay.h:166-195), then walk them:
// F |= key of the F site, R |= key of the R site (Word::operator|, word.h:421-440: the union over the oligo's own slots), each
// accepted only while the degeneracy stays within opt.degen and PCR::is_valid (with the homodimer test) holds; then, while the
// heterodimer Tm of the assay exceeds opt.max_dimer, the single-base reduction of either oligo that lowers it most.
//
// Here: the candidate amplicons of ALL assays come from one pass of the amplicon kernels in the reference's order
// (candidate_amplicons + order_amplicons, the machinery of the background screen's ordered path) with the site keys gathered by
// k_amp_words; identities, the sort and the two greedy walks run on the host (they are sequential per oligo by definition), and
// the thermodynamics they ask for go to the device in ROUNDS over all assays: a walk proposes, beside its next candidate word,
// the candidates that follow if that one is rejected (its state does not change then), every distinct word of a round is one
// pcr_thermo job, and the answers are remembered -- so a walk costs about one launch per ACCEPTED union, not one per amplicon.
// Ties of the sort: std::sort is not stable; the product uses the same libstdc++ algorithm on the same initial order (the
// reference's amplicon order), which is what makes it reproduce the reference's permutation.

namespace {

__global__ void k_amp_words(const AmpRec *__restrict__ recs, uint32_t n, const DevEntry *__restrict__ db, uint4 *__restrict__ out)
{
	const uint32_t k = blockIdx.x*blockDim.x + threadIdx.x;
	if(k >= n) return;
	const AmpRec r = recs[k];
	const Planes f = db[r.f_entry].w, q = db[r.r_entry].w;
	out[2*(size_t)k] = make_uint4(f.a, f.c, f.g, f.t);
	out[2*(size_t)k + 1] = make_uint4(q.a, q.c, q.g, q.t);
}

inline bool h_nondegen(unsigned v) { return v == 1 || v == 2 || v == 4 || v == 8; }                  // base_table.h:125
inline int h_taq_idx(unsigned v) { return (v == 2) ? 0 : (v == 4) ? 1 : (v == 1) ? 2 : 3; }          // word.cpp:233

// update_identity for one (oligo, key), optimize.cpp:209-261 (the device's identity(), pcr_screen.inc, on the host)
float host_identity(const Planes &o, const Planes &key, bool use_taq)
{
	const unsigned len = (unsigned)pcrhost::planes_size(o);
	const float norm = (len > 0) ? (float)(1.0/len) : 0.0f;                           // :221
	const unsigned cnt = (unsigned)__builtin_popcount((key.a & o.a) | (key.c & o.c) | (key.g & o.g) | (key.t & o.t));
	float id = (float)cnt*norm;
	if(use_taq){
		const int last = pcrhost::planes_stop(o), pen = last - 1;
		if(pen >= 0){
			const unsigned p1 = pcrhost::planes_nibble(o, pen), p2 = pcrhost::planes_nibble(o, last);
			const unsigned t1 = pcrhost::planes_nibble(key, pen), t2 = pcrhost::planes_nibble(key, last);
			if(h_nondegen(p1) && h_nondegen(p2) && h_nondegen(t1) && h_nondegen(t2))
				id *= std::min(1.0f, h_taq_mama[16*(4*h_taq_idx(t2) + h_taq_idx(t1)) + (4*h_taq_idx(p2) + h_taq_idx(p1))]);
		}
	}
	return id;
}

// Word::operator| (word.h:421-440): the union over the LEFT word's slots start() .. stop()
inline Planes planes_union(const Planes &w, const Planes &key)
{
	const int first = pcrhost::planes_start(w), last = pcrhost::planes_stop(w);
	if(last < first) return w;
	const uint32_t span = (last - first == 31) ? 0xFFFFFFFFu : (((1u << (last - first + 1)) - 1u) << first);
	Planes r = w;
	r.a |= key.a & span; r.c |= key.c & span; r.g |= key.g & span; r.t |= key.t & span;
	return r;
}

struct DegAmp { Planes fkey, rkey; float score; };

// one candidate amplicon with its sort key and site words, as the ranks of a sharded call exchange them
struct ShardAmp { uint32_t pair, orient; uint64_t seq; /* global sequence index */ uint4 f, r; };
static_assert(sizeof(ShardAmp) == 48, "exchanged as raw bytes");

// The candidate amplicons of every assay on this handle's targets, in the reference's order (candidate_amplicons +
// order_amplicons: by pair, orientation, sequence, plus site, minus site), with the words of their sites; seq_base is added to
// the sequence indices (the shard's first row).
int degenerate_amplicons(pcr_ctx *ctx, SeqSet &S, const pcr_pair *assays, uint32_t n, const pcr_optimize_args *o, uint64_t seq_base, std::vector<ShardAmp> &out)
{
	out.clear();
	if(!S.have_db){ g_err = "pcr_make_degenerate: no word DB (call pcr_select_words on the targets first)"; return PCR_ERR_STATE; }
	int rc;
	if((rc = ensure_touched(ctx, S)) != PCR_OK) return rc;
	if(!S.n_entries) return PCR_OK;
	uint32_t n_amp = 0;
	if((rc = candidate_amplicons(ctx, S, assays, n, o->target.collect_threshold, o->target.amp_min, o->target.amp_max, &n_amp)) != PCR_OK) return rc;
	if(!n_amp) return PCR_OK;
	const AmpRec *d_recs = nullptr; const uint32_t *d_pair_start = nullptr;
	if((rc = order_amplicons(ctx, S, n_amp, n, &d_recs, &d_pair_start)) != PCR_OK) return rc;
	DevBuf<uint4> d_words;
	if((rc = d_words.ensure(2*(size_t)n_amp)) != PCR_OK) return rc;
	hipLaunchKernelGGL(k_amp_words, dim3((n_amp + 255)/256), dim3(256), 0, ctx->stream, d_recs, n_amp, S.db.p, d_words.p);
	std::vector<AmpRec> recs(n_amp); std::vector<uint4> words(2*(size_t)n_amp);
	hipError_t e = hipGetLastError();
	if(e == hipSuccess) e = hipMemcpyAsync(recs.data(), d_recs, (size_t)n_amp*sizeof(AmpRec), hipMemcpyDeviceToHost, ctx->stream);
	if(e == hipSuccess) e = hipMemcpyAsync(words.data(), d_words.p, 2*(size_t)n_amp*sizeof(uint4), hipMemcpyDeviceToHost, ctx->stream);
	if(e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
	if(e != hipSuccess){ g_err = std::string("pcr_make_degenerate: ") + hipGetErrorString(e); return PCR_ERR_DEVICE; }
	for(uint32_t k = 0;k < n_amp;++k){                                            // (sorted by pair, inside a pair in the reference's order)
		if(recs[k].pair >= n) continue;
		ShardAmp a;
		a.pair = recs[k].pair; a.orient = (recs[k].f_entry > recs[k].r_entry) ? 1u : 0u; a.seq = seq_base + recs[k].seq;   // (k_amp_keys' orientation)
		a.f = words[2*(size_t)k]; a.r = words[2*(size_t)k + 1];
		out.push_back(a);
	}
	return PCR_OK;
}

// Sharded: every rank's list (local_rc: how this rank's collection went) -> the whole list on every rank, in the reference's order.
// Each rank's list is sorted by (pair, orientation, sequence, sites) and the ranks hold disjoint ascending sequence ranges, so a
// stable sort of the rank-order concatenation by (pair, orientation, sequence) is the merge.  One size all-gather, then one padded
// all-gather of the records.
int shard_gather_amplicons(pcr_ctx *ctx, int local_rc, std::vector<ShardAmp> &amps)
{
	pcr_comm *c = ctx->shard_comm;
	const size_t W = (size_t)c->world;
	const uint64_t me[2] = {local_rc != PCR_OK ? sh_fail_bit(local_rc) : 0ull, local_rc != PCR_OK ? 0ull : (uint64_t)amps.size()};
	std::vector<uint64_t> sizes(2*W);
	int rc = sh_allgather_host(ctx, c, me, sizeof(me), sizes.data());
	if(rc != PCR_OK) return rc;
	uint64_t st = 0, most = 0;
	for(size_t r = 0;r < W;++r){ st |= sizes[2*r]; most = std::max(most, sizes[2*r + 1]); }
	if(st) return sh_status_rc(st, local_rc, "pcr_make_degenerate");
	std::vector<ShardAmp> send((size_t)most), all((size_t)most*W);
	if(most){
		std::copy(amps.begin(), amps.end(), send.begin());
		if((rc = sh_allgather_host(ctx, c, send.data(), most*sizeof(ShardAmp), all.data())) != PCR_OK) return rc;
	}
	amps.clear();
	for(size_t r = 0;r < W;++r) amps.insert(amps.end(), all.begin() + r*most, all.begin() + r*most + sizes[2*r + 1]);
	std::stable_sort(amps.begin(), amps.end(), [](const ShardAmp &l, const ShardAmp &r){
		return (l.pair != r.pair) ? l.pair < r.pair : (l.orient != r.orient) ? l.orient < r.orient : l.seq < r.seq; });
	return PCR_OK;
}

} // namespace

extern "C" int pcr_make_degenerate(pcr_ctx *ctx, pcr_pair *assays, uint32_t n, const pcr_optimize_args *o, uint8_t *valid_out)
{
	if(!ctx){ g_err = "pcr_make_degenerate: bad argument"; return PCR_ERR_ARG; }
	const bool args_ok = o && !(n && (!assays || !valid_out));
	if(!args_ok) g_err = "pcr_make_degenerate: bad argument";
	if(ctx->shard_comm){                                                           // sharded: every rank enters with the same call, or none goes on
		int rc0 = args_ok ? enter_device(ctx) : PCR_ERR_ARG;
		rc0 = shard_agree(ctx, rc0 == PCR_OK ? opt_fingerprint(3, assays, n, o, nullptr, 0) : 0, rc0, "pcr_make_degenerate");
		if(rc0 != PCR_OK) return rc0;
	}
	if(!args_ok) return PCR_ERR_ARG;
	DRAIN(ctx);
	HIP_TRY(hipSetDevice(ctx->device));
	if(n == 0) return PCR_OK;
	SeqSet &S = ctx->sets[PCR_SET_TARGET];
	int rc;
	const bool use_taq = o->target.use_taq_mama != 0;
	// ---- the candidate amplicons of every assay in the reference's order, with the words of their sites (sharded: every rank's,
	// merged; the rest of the call is local and the same on every rank)
	std::vector<ShardAmp> cand;
	rc = degenerate_amplicons(ctx, S, assays, n, o, ctx->shard_comm ? ctx->shard_first : 0, cand);
	if(ctx->shard_comm) rc = shard_gather_amplicons(ctx, rc, cand);
	if(rc != PCR_OK) return rc;
	std::vector<std::vector<DegAmp> > amps(n);
	for(const ShardAmp &x : cand){
		DegAmp a;
		a.fkey = Planes{x.f.x, x.f.y, x.f.z, x.f.w};
		a.rkey = Planes{x.r.x, x.r.y, x.r.z, x.r.w};
		a.score = 0.0f;
		amps[x.pair].push_back(a);
	}
	// ---- identities, score, sort_target_candidates (assay.h:166-195)
	std::vector<Planes> F(n), R(n);
	for(uint32_t a = 0;a < n;++a){
		F[a] = pcrhost::planes_of_word(assays[a].f.w); R[a] = pcrhost::planes_of_word(assays[a].r.w);
		for(DegAmp &x : amps[a]) x.score = sqrtf(host_identity(F[a], x.fkey, use_taq)*host_identity(R[a], x.rkey, use_taq));
		std::sort(amps[a].begin(), amps[a].end(), [](const DegAmp &l, const DegAmp &r){ return l.score > r.score; });   // descending; ties as std::sort leaves them
	}
	// ---- maximize_degeneracy, first part (pcr_assay.cpp:113-130): two independent walks per assay
	struct Walk { Planes w; size_t pos; uint32_t assay; int side; bool done; };
	std::vector<Walk> walks;
	for(uint32_t a = 0;a < n;++a){ walks.push_back(Walk{F[a], 0, a, 0, false}); walks.push_back(Walk{R[a], 0, a, 1, false}); }
	ValidCache cache;                                                             // is_valid WITH the homodimer test (valid_pcr.cpp:5-45, check dimer = true)
	const pcr_thermo_args targs = o->thermo;
	auto key_of = [&](const Walk &k, size_t q) -> const Planes & { return k.side ? amps[k.assay][q].rkey : amps[k.assay][q].fkey; };
	constexpr size_t SPECULATE = 48;                                              // candidates a walk proposes per round beyond its next one
	for(int round = 0;round < 100000;++round){
		std::vector<pcr_word128> ask;
		ValidCache asked;                                                          // words already in this round's list
		for(Walk &k : walks){
			if(k.done) continue;
			const size_t n_a = amps[k.assay].size();
			while(k.pos < n_a){
				const Planes c = planes_union(k.w, key_of(k, k.pos));
				if(planes_eq(c, k.w) || pcrhost::planes_degeneracy(c) > o->max_degen){ ++k.pos; continue; }   // nothing new (is_valid's answer cannot change the oligo) / too degenerate
				const int v = cache.find(c);
				if(v < 0) break;
				if(v) k.w = c;                                                      // pcr_assay.cpp:122-128
				++k.pos;
			}
			if(k.pos >= n_a){ k.done = true; continue; }
			size_t proposed = 0;
			for(size_t q = k.pos;q < n_a && proposed <= SPECULATE;++q){             // the next candidate and those that follow if the ones before them are rejected
				const Planes c = planes_union(k.w, key_of(k, q));
				if(planes_eq(c, k.w) || pcrhost::planes_degeneracy(c) > o->max_degen) continue;
				if(cache.find(c) >= 0 || asked.find(c) >= 0) continue;
				asked.put(c, true);
				ask.push_back(word_of(c));
				++proposed;
			}
		}
		if(ask.empty()) break;
		std::vector<pcr_thermo_result> res(ask.size());
		if((rc = pcr_thermo(ctx, ask.data(), (uint32_t)ask.size(), 1, &targs, res.data())) != PCR_OK) return rc;
		for(size_t i = 0;i < ask.size();++i) cache.put(pcrhost::planes_of_word(ask[i].w), res[i].valid != 0);
	}
	for(const Walk &k : walks){ if(k.side) R[k.assay] = k.w; else F[k.assay] = k.w; }
	// ---- second part (:132-229): while the heterodimer Tm exceeds max_dimer, the single-base reduction that lowers it most
	std::vector<float> tm(n);
	{
		std::vector<pcr_pair> pp(n);
		for(uint32_t a = 0;a < n;++a){ pp[a].f = word_of(F[a]); pp[a].r = word_of(R[a]); }
		if((rc = pcr_dimer(ctx, pp.data(), n, &targs, tm.data())) != PCR_OK) return rc;
	}
	std::vector<uint8_t> live(n, 0);
	for(uint32_t a = 0;a < n;++a){ valid_out[a] = 1; live[a] = tm[a] > targs.max_dimer; }
	auto reductions = [](const Planes &w, std::vector<Planes> &out){
		const int first = pcrhost::planes_start(w), last = pcrhost::planes_stop(w);
		for(int i = first;i <= last;++i){
			const unsigned curr = pcrhost::planes_nibble(w, i);
			for(unsigned b = 1;b <= 8;b <<= 1){                                     // Base::A .. Base::T
				const unsigned d = curr & ~b;
				if(!d || d == curr) continue;                                      // a single base, or a base the slot does not hold
				Planes v = w;
				const uint32_t m = ~(1u << i);
				if(b == 1) v.a &= m; else if(b == 2) v.c &= m; else if(b == 4) v.g &= m; else v.t &= m;
				out.push_back(v);
			}
		}
	};
	for(int round = 0;round < 4096;++round){
		std::vector<pcr_pair> cand; std::vector<uint32_t> first(n + 1, 0), n_f(n, 0);
		std::vector<Planes> tmp;
		bool any = false;
		for(uint32_t a = 0;a < n;++a){
			first[a] = (uint32_t)cand.size();
			if(!live[a]) continue;
			any = true;
			tmp.clear(); reductions(F[a], tmp); n_f[a] = (uint32_t)tmp.size();
			for(const Planes &v : tmp){ pcr_pair p; p.f = word_of(v); p.r = word_of(R[a]); cand.push_back(p); }
			tmp.clear(); reductions(R[a], tmp);
			for(const Planes &v : tmp){ pcr_pair p; p.f = word_of(F[a]); p.r = word_of(v); cand.push_back(p); }
		}
		first[n] = (uint32_t)cand.size();
		if(!any) break;
		std::vector<float> ctm(cand.size() + 1);
		if(!cand.empty() && (rc = pcr_dimer(ctx, cand.data(), (uint32_t)cand.size(), &targs, ctm.data())) != PCR_OK) return rc;
		for(uint32_t a = 0;a < n;++a){
			if(!live[a]) continue;
			float curr = 1.0e6f; int best = -1;
			for(uint32_t k = first[a];k < first[a + 1];++k){ if(ctm[k] < curr){ curr = ctm[k]; best = (int)k; } }   // the first of the lowest
			if(best < 0){ valid_out[a] = 0; live[a] = 0; continue; }                // non-degenerate and still over the limit (:219-223)
			if((uint32_t)best - first[a] < n_f[a]) F[a] = pcrhost::planes_of_word(cand[(size_t)best].f.w); else R[a] = pcrhost::planes_of_word(cand[(size_t)best].r.w);
			tm[a] = curr;
			if(!(curr > targs.max_dimer)) live[a] = 0;
		}
	}
	for(uint32_t a = 0;a < n;++a){ assays[a].f = word_of(F[a]); assays[a].r = word_of(R[a]); }
	return PCR_OK;
}
