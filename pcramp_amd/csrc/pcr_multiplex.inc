// The multiplex terms of the local search: multiplex background coverage, oligo reuse, amplicons of an assay.
//
// Unlike the target and background coverages this one counts KEYS: the multiplex background DB is every
// word Sequence::pack emits for the amplicons of the assays accepted so far (main.cpp:989-1001: pack only,
// no select_words, no G+C filter), the candidate keys of an assay are those its forward primer / its reverse
// primer matches at background_threshold (match_words, pcr_assay.cpp:71-102), and the coverage is the number
// of distinct candidate keys whose identity with F or with R reaches the threshold (pcr_assay.cpp:304-336).
// The amplicon set is small and changes once per accepted assay, so the key table is built on the host from
// the same window model the scan kernels use (regular windows + irregular words, pcr_host.hpp) and kept on
// the device; k_key_coverage evaluates all trial words of a move over it in one launch.
// Included by pcr_entry_sw_thermo.inc.

namespace {

__global__ void k_key_coverage(const Planes *__restrict__ keys, uint32_t n_keys, const OligoDev *__restrict__ base /* F, R */,
	const OligoDev *__restrict__ variants, uint32_t n_variants, int side, float thr, int use_taq, uint32_t *__restrict__ count)
{
	const uint32_t k = blockIdx.x*blockDim.x + threadIdx.x;
	if(k >= n_keys) return;
	const Planes key = keys[k];
	const OligoDev F = base[0], R = base[1];
	// collect_multiplex_background_candidates: the key is in the f map / the r map
	const bool in_f = (uint32_t)__popc((key.a & F.m.a) | (key.c & F.m.c) | (key.g & F.m.g) | (key.t & F.m.t)) >= F.floor2;
	const bool in_r = (uint32_t)__popc((key.a & R.m.a) | (key.c & R.m.c) | (key.g & R.m.g) | (key.t & R.m.t)) >= R.floor2;
	if(!in_f && !in_r) return;
	const bool in_edit = (side == 0) ? in_f : in_r, in_other = (side == 0) ? in_r : in_f;
	const bool other_ok = in_other && identity((side == 0) ? R : F, key, use_taq) >= thr;   // the map of the oligo that is not edited
	for(uint32_t v = 0;v < n_variants;++v){
		if(other_ok || (in_edit && identity(variants[v], key, use_taq) >= thr)) atomicAdd(&count[v], 1u);   // each key counts once (:313-333)
	}
}

// PCR::collect_unique_amplicons (pcr_assay.cpp:756-813) / extract_amplicon_seq (:443-542) over the word DB of the
// last select: a thread owns a plus-strand DB entry matched by the plus-role oligo (mask from k_match_few at
// threshold^2) and sweeps the minus-strand entries after it.  No identity test and no end clamp here (unlike
// the amplicon screen): binding-site overlap, amplicon length, and an EOS-free inner stretch (the non-primer part
// with MULTIPLEX_AMPLICON_PADDING, spelled 4 bases further into the minus primer than its name says, :492-494).
__global__ void k_collect_amplicons(const DevEntry *__restrict__ db, uint32_t n, uint32_t cap, const uint32_t *__restrict__ touched,
	const uint32_t *__restrict__ seg_hi, const uint32_t *__restrict__ mask, const OligoDev *__restrict__ base /* F, R */,
	const uint4 *__restrict__ planes, const uint64_t *__restrict__ blk_off, const uint64_t *__restrict__ len,
	const uint8_t *__restrict__ active, const uint8_t *__restrict__ has_eos, int32_t amp_min, int32_t amp_max,
	pcr_amplicon *__restrict__ out, uint32_t out_cap, uint32_t *__restrict__ count)
{
	uint32_t i;
	if(!db_slot(blockIdx.x*blockDim.x + threadIdx.x, n, cap, touched, seg_hi, i)) return;
	const uint32_t mi = mask[i];
	if(!(mi & 3u)) return;
	const DevEntry ei = db[i];
	if(ei.strand != 1 || !active[ei.seq]) return;                                // find_oligo_match: strand, active (optimize.cpp:277-285)
	const uint32_t hi = seg_hi[ei.seq];
	const int32_t L = (int32_t)len[ei.seq];
	const uint64_t blk_base = blk_off[ei.seq];
	const bool eos = has_eos[ei.seq] != 0;
	const OligoDev F = base[0], R = base[1];
	for(uint32_t j = i + 1;j < hi;++j){
		const DevEntry ej = db[j];
		if(ej.loc - ei.loc > amp_max + 128) break;
		if(ej.strand != 2) continue;
		const uint32_t mj = mask[j];
		for(int orient = 0;orient < 2;++orient){
			if(!((orient == 0) ? (mi & (mj >> 1) & 1u) : ((mi >> 1) & mj & 1u))) continue;
			const OligoDev &P = (orient == 0) ? F : R;                           // plus-role oligo
			const OligoDev &M = (orient == 0) ? R : F;                           // minus-role oligo
			const int32_t p5 = ei.loc + P.start, p3 = ei.loc + P.stop;           // template_loc5/3, sequence.h:57-75
			const int32_t m5 = ej.loc - M.stop, m3 = ej.loc - M.start;
			if(p3 >= m5) continue;                                               // :468-471
			const int32_t amp_len = m3 - p5 + 1;
			if(amp_len < amp_min || amp_len > amp_max) continue;                 // :477-484
			const int32_t in_start = p3 + 1 - 4;                                 // :489-490
			const int32_t in_len = m5 - in_start + 8;                            // :492-494
			if(in_start < 0 || in_len < 0 || in_start + in_len > L) continue;    // reads past the sequence there; no amplicon here
			if(eos && has_split(planes, blk_base, in_start, in_len)) continue;   // :504-521
			const uint32_t k = atomicAdd(count, 1u);
			if(k < out_cap){
				pcr_amplicon a;
				a.sequence = ei.seq; a.begin = p5; a.end = m3; a.inner_start = in_start; a.inner_length = in_len; a.orientation = (uint32_t)orient;
				out[k] = a;
			}
		}
	}
}

struct PlanesLess {
	bool operator()(const Planes &x, const Planes &y) const
	{
		if(x.a != y.a) return x.a < y.a;
		if(x.c != y.c) return x.c < y.c;
		if(x.g != y.g) return x.g < y.g;
		return x.t < y.t;
	}
};

} // namespace

extern "C" {

// ---- the oligo-reuse term of the multiplex Score (host arithmetic)
float pcr_host_max_overlap(const pcr_word128 *a, const pcr_word128 *b)
{
	if(!a || !b) return 0.0f;
	return pcrhost::max_overlap(pcrhost::planes_of_word(a->w), pcrhost::planes_of_word(b->w));
}

int pcr_host_pool_overlaps(const pcr_word128 *words, uint32_t n, const pcr_pair *pool, uint32_t n_pool, float *out)
{
	if((n && (!words || !out)) || (n_pool && !pool)){ g_err = "pcr_host_pool_overlaps: bad argument"; return PCR_ERR_ARG; }
	std::vector<Planes> pp(2*(size_t)n_pool);
	for(uint32_t i = 0;i < n_pool;++i){ pp[2*i] = pcrhost::planes_of_word(pool[i].f.w); pp[2*i + 1] = pcrhost::planes_of_word(pool[i].r.w); }
	for(uint32_t k = 0;k < n;++k){
		const Planes w = pcrhost::planes_of_word(words[k].w);
		float best = 0.0f;
		for(const Planes &p : pp) best = std::max(best, pcrhost::max_overlap(w, p));
		out[k] = best;
	}
	return PCR_OK;
}

float pcr_host_oligo_overlap(const pcr_pair *assay, const pcr_pair *pool, uint32_t n_pool)
{
	if(!assay || (n_pool && !pool)) return 0.0f;
	std::vector<Planes> pp(2*(size_t)n_pool);
	for(uint32_t i = 0;i < n_pool;++i){ pp[2*i] = pcrhost::planes_of_word(pool[i].f.w); pp[2*i + 1] = pcrhost::planes_of_word(pool[i].r.w); }
	return pcrhost::oligo_overlap(pcrhost::planes_of_word(assay->f.w), pcrhost::planes_of_word(assay->r.w), pp.data(), n_pool);
}

// ---- the multiplex background
int pcr_multiplex_load(pcr_ctx *ctx, const uint8_t *packed4, const uint64_t *byte_offsets, const uint64_t *lengths, uint32_t n,
	uint32_t min_oligo_length, uint64_t *n_keys_out)
{
	if(!ctx || (n && (!packed4 || !byte_offsets || !lengths)) || min_oligo_length == 0 || min_oligo_length > 32){
		g_err = "pcr_multiplex_load: bad argument"; return PCR_ERR_ARG;
	}
	FLUSH(ctx);
	HIP_TRY(hipSetDevice(ctx->device));
	pcrhost::PackFilter filt;
	filt.max_degen = ctx->params.pack_max_degen;
	filt.set_gc(0.0f, 1.0f);                                                     // main.cpp:994: no G+C filter for the amplicons
	std::vector<Planes> keys;
	std::vector<pcrhost::IrrEntry> irr;
	for(uint32_t s = 0;s < n;++s){
		const uint64_t L = lengths[s];
		std::vector<uint8_t> buf(packed4 + byte_offsets[s], packed4 + byte_offsets[s] + (L + 1)/2);
		if((L & 1) && !buf.empty()) buf.back() &= 0xF0;                          // pad nibble = EOS (sequence.cpp:21)
		pcrhost::PackedSeq q; q.buf = buf.data(); q.len = L;
		// regular windows: 32 non-EOS slots within the degeneracy bound -> the window and its reverse complement
		for(uint64_t p = 0;p + 32 <= L;++p){
			uint64_t w[2] = {0, 0};
			unsigned n2 = 0, n3 = 0, n4 = 0;
			bool ok = true;
			for(int k = 0;k < 32;++k){
				const unsigned v = q.at(p + k);
				if(v == 0){ ok = false; break; }
				const int d = __builtin_popcount(v);
				n2 += (d == 2); n3 += (d == 3); n4 += (d == 4);
				pcrhost::word_set(w, k, v);
			}
			if(!ok || pcrhost::degeneracy_exceeds(n2, n3, n4, filt.max_degen)) continue;
			const Planes pl = pcrhost::planes_of_word(w);
			keys.push_back(pl);
			keys.push_back(pcrhost::planes_revcomp(pl));
		}
		// irregular words: the centred partial words at the ends and around EOS, of at least min_oligo_length bases
		irr.clear();
		if(!pcrhost::irregular_words(q, filt, irr)){ g_err = "pcr_multiplex_load: irregular word overflow"; return PCR_ERR_CAPACITY; }
		for(const pcrhost::IrrEntry &e : irr){ if(e.cws >= min_oligo_length) keys.push_back(e.w); }
	}
	std::sort(keys.begin(), keys.end(), PlanesLess());                            // keys(): the unique words (pcramp.h:231-256)
	keys.erase(std::unique(keys.begin(), keys.end(), [](const Planes &x, const Planes &y){ return x.a == y.a && x.c == y.c && x.g == y.g && x.t == y.t; }), keys.end());
	int rc;
	if((rc = ctx->mx_keys.ensure(keys.size() + 1)) != PCR_OK) return rc;
	if(!keys.empty()) HIP_TRY(hipMemcpy(ctx->mx_keys.p, keys.data(), keys.size()*sizeof(Planes), hipMemcpyHostToDevice));
	ctx->mx_n_keys = (uint32_t)keys.size();
	if(n_keys_out) *n_keys_out = keys.size();
	return PCR_OK;
}

int pcr_multiplex_coverage(pcr_ctx *ctx, const pcr_pair *base, int side, const pcr_word128 *variants, uint32_t n_variants,
	float background_threshold, int use_taq_mama, float *coverage)
{
	if(!ctx || !base || (side != 0 && side != 1) || (n_variants && (!variants || !coverage))){ g_err = "pcr_multiplex_coverage: bad argument"; return PCR_ERR_ARG; }
	FLUSH(ctx);
	HIP_TRY(hipSetDevice(ctx->device));
	for(uint32_t v = 0;v < n_variants;++v) coverage[v] = 0.0f;
	if(ctx->mx_n_keys == 0 || n_variants == 0) return PCR_OK;                    // pcr_assay.cpp:75-77, :306-308
	std::vector<OligoDev> ol(2 + (size_t)n_variants);
	fill_oligo(ol[0], base->f.w, background_threshold);                           // match_words at background_threshold, NOT squared (pcr_assay.cpp:86,96)
	fill_oligo(ol[1], base->r.w, background_threshold);
	for(uint32_t v = 0;v < n_variants;++v){
		if((variants[v].w[0] | variants[v].w[1]) == 0){ g_err = "pcr_multiplex_coverage: empty trial oligo"; return PCR_ERR_ARG; }
		fill_oligo(ol[2 + v], variants[v].w, background_threshold);
	}
	int rc;
	if((rc = ctx->mx_count.ensure((size_t)n_variants + 4)) != PCR_OK) return rc;
	Stager st(ctx);
	if((rc = st.begin(ol.size()*sizeof(OligoDev) + 64)) != PCR_OK) return rc;
	const OligoDev *d_ol = st.put(ol.data(), ol.size());
	if((rc = st.ship(ctx->mx_count.p, (size_t)n_variants*sizeof(uint32_t))) != PCR_OK) return rc;
	hipLaunchKernelGGL(k_key_coverage, dim3((ctx->mx_n_keys + 255)/256), dim3(256), 0, ctx->stream, ctx->mx_keys.p, ctx->mx_n_keys, d_ol, d_ol + 2,
		n_variants, side, background_threshold, use_taq_mama, ctx->mx_count.p);
	HIP_TRY(hipGetLastError());
	const uint8_t *back[3];
	if((rc = return_to_host(ctx, ctx->mx_count.p, (size_t)n_variants*sizeof(uint32_t), nullptr, 0, nullptr, 0, back)) != PCR_OK) return rc;
	const uint32_t *cnt = (const uint32_t *)back[0];
	for(uint32_t v = 0;v < n_variants;++v) coverage[v] = (float)(double)cnt[v];   // "each multiplex background gets weight 1.0", summed in double
	return PCR_OK;
}

int64_t pcr_collect_amplicons(pcr_ctx *ctx, pcr_set which, const pcr_pair *pair, float threshold, int32_t amp_min, int32_t amp_max,
	pcr_amplicon *out, uint64_t cap)
{
	if(!set_ok(which)){ g_err = "pcr_collect_amplicons: unknown sequence set"; return PCR_ERR_ARG; }
	if(!ctx || !pair || (which != PCR_SET_TARGET && which != PCR_SET_BACKGROUND) || (cap && !out)){ g_err = "pcr_collect_amplicons: bad argument"; return PCR_ERR_ARG; }
	{ const int drc = drain(ctx); if(drc != PCR_OK) return drc; }
	HIP_TRY(hipSetDevice(ctx->device));
	SeqSet &S = ctx->sets[which];
	if(!S.have_db){ g_err = "pcr_collect_amplicons: no word DB (call pcr_select_words first)"; return PCR_ERR_STATE; }
	{ const int erc = ensure_touched(ctx, S); if(erc != PCR_OK) return erc; }
	if(S.n_entries == 0) return 0;
	int rc;
	std::vector<OligoDev> ol(2);
	const float thr2 = threshold*threshold;                                      // pcr_assay.cpp:775-776
	fill_oligo(ol[0], pair->f.w, thr2);
	fill_oligo(ol[1], pair->r.w, thr2);
	const uint32_t out_cap = (uint32_t)std::min<uint64_t>(cap, 1u << 24);
	if((rc = ctx->mx_count.ensure(8)) != PCR_OK) return rc;
	if((rc = ctx->mx_amp.ensure((size_t)out_cap + 1)) != PCR_OK) return rc;
	if((rc = ctx->mask.ensure((size_t)S.n_slots)) != PCR_OK) return rc;
	Stager st(ctx);
	if((rc = st.begin(ol.size()*sizeof(OligoDev) + 64)) != PCR_OK) return rc;
	const OligoDev *d_ol = st.put(ol.data(), ol.size());
	if((rc = st.ship(ctx->mx_count.p, 16)) != PCR_OK) return rc;
	const uint32_t n_db = S.n_touched*S.db_cap;
	hipLaunchKernelGGL(k_match_few, dim3((n_db + 255)/256), dim3(256), 0, ctx->stream, S.db.p, n_db, S.db_cap, S.touched.p, S.d_seg_hi, d_ol, 2u,
		ctx->mask.p, (uint32_t *)nullptr);
	HIP_TRY(hipGetLastError());
	hipLaunchKernelGGL(k_collect_amplicons, dim3((n_db + 127)/128), dim3(128), 0, ctx->stream, S.db.p, n_db, S.db_cap, S.touched.p, S.d_seg_hi, ctx->mask.p,
		d_ol, S.planes.p, S.d_blk_off.p, S.d_len.p, S.d_active.p, S.d_has_eos.p, amp_min, amp_max, ctx->mx_amp.p, out_cap, ctx->mx_count.p);
	HIP_TRY(hipGetLastError());
	const uint8_t *back[3];
	if((rc = return_to_host(ctx, ctx->mx_count.p, 16, nullptr, 0, nullptr, 0, back)) != PCR_OK) return rc;
	const uint32_t found = *(const uint32_t *)back[0];
	const uint32_t got = std::min(found, out_cap);
	if(got){
		if((rc = return_to_host(ctx, ctx->mx_amp.p, (size_t)got*sizeof(pcr_amplicon), nullptr, 0, nullptr, 0, back)) != PCR_OK) return rc;
		memcpy(out, back[0], (size_t)got*sizeof(pcr_amplicon));
		std::sort(out, out + got, [](const pcr_amplicon &x, const pcr_amplicon &y){                 // a stable order for the caller
			if(x.orientation != y.orientation) return x.orientation < y.orientation;
			if(x.sequence != y.sequence) return x.sequence < y.sequence;
			if(x.begin != y.begin) return x.begin < y.begin;
			return x.end < y.end;
		});
	}
	return (int64_t)found;
}

} // extern "C"
