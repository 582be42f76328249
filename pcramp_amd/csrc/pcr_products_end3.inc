// Products of a primer pool under a 3'-end extension rule (pcr_pool_products_end3; included by pcr_device.hip after
// pcr_products_tm.inc, whose stages, pair table and bit rows it shares).
//
// pcr_pool_products_tm decides from the slots matching over the whole oligo and from the duplex Tm; where the mismatches lie is
// not looked at.  A product's two sites are two item indices, so what the rule needs of a site is stored per ITEM, beside item_tm[]:
//   1. item_count / item_fill (pcr_pool.inc): the items and item_off.
//   2. k_item_end3: a thread per item; site_pick gives the entry pcr_site_tm reads the site from, and the item's ItemEnd (8 bytes) is
//      clamp3, the mismatches among the last `window` slots, the oligo's length and update_identity's score (identity(),
//      pcr_screen.inc, as it stands: the one place the TaqMAMA factor is applied).  Indexed by item; nothing else is read per site.
//   3. melt_items (pcr_site_tm.inc) -> item_tm[], only with thermodynamics (args != NULL) and where pcr_pool_products_tm melts.
//   4. k_end3_join<false> / <true>: k_products_join's walk (join_walk), its floor, then the rule on the two ItemEnd.  The count pass
//      counts the kept products per item and, in a second per-item counter, those past the floor before the rule (summed by
//      rocprim::reduce: integers, no atomics), and sets the bits of the kept products.  The emit pass writes the 64-byte records.
//   5. The record order: product_order (pcr_pool.inc).
// A plus site that fails its own half of the rule keeps no product: it walks nothing (in the count pass only where the before-rule
// count is not asked for).  Items, jobs and Tm live in pcr_ctx::shared; the ItemEnd array and the join's buffers are pcr_ctx::pe3_*.
// The files included after this one (pcr_anneal_profile.inc, pcr_pool_conflicts.inc, pcr_probe_hits.inc) apply the same rule in
// their joins through end3_rule_of, end3_norms, end3_items (step 2 into pe3_end), end3_site_ok and end3_product_ok below.
#include <rocprim/device/device_reduce.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

namespace {

struct alignas(8) ItemEnd { uint8_t clamp3, end_mismatch, length, pad; float id; };   // of the item's site: one 8-byte load
struct End3Rule { uint32_t min_clamp3, window, max_end_mismatch; float ident_threshold; };
struct End3Widen { __device__ uint64_t operator()(uint32_t v) const { return (uint64_t)v; } };

// Item k -> item_end[k], from the entry site_pick chooses (pcr_site_tm's, so the numbers are those of the site's pcr_site_variants
// record).  norm[o] = float(1.0/length) of oligo o, from the host as OligoDev's.
__global__ __launch_bounds__(POOL_THREADS) void k_item_end3(const DevEntry *__restrict__ db, uint32_t cap, const uint32_t *__restrict__ touched,
	const uint32_t *__restrict__ seg_hi, const uint2 *__restrict__ items, uint32_t n_items, const PoolOligo *__restrict__ oligos,
	const float *__restrict__ norm, uint32_t window, int use_taq, ItemEnd *__restrict__ item_end)
{
	const uint32_t k = blockIdx.x*blockDim.x + threadIdx.x;
	if(k >= n_items) return;
	const uint2 it = items[k];
	const PoolOligo o = oligos[it.y];
	const uint32_t slot = site_slot(it.x, cap, touched);
	const DevEntry en = site_pick(db, slot, seg_hi[db[slot].seq], o, site_window(o.start, o.stop));
	const uint32_t hit = (en.w.a & o.m.a) | (en.w.c & o.m.c) | (en.w.g & o.m.g) | (en.w.t & o.m.t);
	const uint32_t upto = (o.stop >= 31) ? 0xFFFFFFFFu : ((1u << (o.stop + 1)) - 1u);
	const uint32_t miss = ~hit & upto & ~((1u << o.start) - 1u);                  // k_sv_records': an empty slot of the word matches nothing
	const uint32_t len = (uint32_t)(o.stop - o.start + 1);                        // 1 .. 32 (no hole: the host refuses it)
	const uint32_t win = min(window, len);
	const uint32_t below = (uint32_t)o.stop + 1u - win;                           // the window is slots below .. stop
	const uint32_t wmask = win ? (upto & ~((below >= 32u) ? 0xFFFFFFFFu : ((1u << below) - 1u))) : 0u;
	OligoDev od;                                                                  // fill_oligo_planes' fields: identity() is called as pcr_amplify calls it
	od.m = o.m; od.floor2 = o.floor2; od.norm = norm[it.y]; od.start = o.start; od.stop = o.stop;
	od.p1 = (o.stop >= 1) ? nibble_at(o.m, o.stop - 1) : 0u; od.p2 = nibble_at(o.m, o.stop);
	ItemEnd r;
	r.clamp3 = (uint8_t)(miss ? (uint32_t)(o.stop - (31 - (int)__builtin_clz(miss))) : len);
	r.end_mismatch = (uint8_t)__popc(miss & wmask);
	r.length = (uint8_t)len; r.pad = 0;
	r.id = identity(od, en.w, use_taq);                                           // (its count is popc(hit): pcr_site.matches)
	item_end[k] = r;
}

__device__ __forceinline__ bool end3_site_ok(const ItemEnd &e, const End3Rule &R)
{
	return (uint32_t)e.clamp3 >= min(R.min_clamp3, (uint32_t)e.length) && !(R.window > 0u && (uint32_t)e.end_mismatch > R.max_end_mismatch);
}

// The rule on a product's two sites, as the keep lambdas of the joins make it after their floor test: the plus half is the caller's
// (plus_ok, tested once per plus item), the minus item's ItemEnd is loaded only past it.
__device__ __forceinline__ bool end3_product_ok(const ItemEnd *__restrict__ item_end, const End3Rule &R, bool plus_ok, const ItemEnd &ep, uint64_t t, ItemEnd &em)
{
	if(!plus_ok) return false;
	em = item_end[t];
	if(!end3_site_ok(em, R)) return false;
	return R.ident_threshold == 0.0f || sqrtf(__fmul_rn(ep.id, em.id)) >= R.ident_threshold;   // sqrtf: see identity()
}

// The caller's rule, checked (NULL: the zero rule); the refusals carry the entry point's name.
int end3_rule_of(const std::string &who, const pcr_end3_rule *rule, End3Rule &R, int &use_taq)
{
	R = End3Rule{0u, 0u, 0u, 0.0f};
	use_taq = 0;
	if(!rule) return PCR_OK;
	if(rule->window > 32u || rule->min_clamp3 > 32u || rule->max_end_mismatch > 32u){ g_err = who + ": window, min_clamp3 or max_end_mismatch above 32"; return PCR_ERR_ARG; }
	if(rule->use_taq_mama != 0 && rule->use_taq_mama != 1){ g_err = who + ": use_taq_mama is neither 0 nor 1"; return PCR_ERR_ARG; }
	if(!std::isfinite(rule->ident_threshold) || !(rule->ident_threshold >= 0.0f && rule->ident_threshold <= 1.0f)){ g_err = who + ": ident_threshold is not finite or outside [0, 1]"; return PCR_ERR_ARG; }
	R.min_clamp3 = rule->min_clamp3; R.window = rule->window; R.max_end_mismatch = rule->max_end_mismatch; R.ident_threshold = rule->ident_threshold;
	use_taq = rule->use_taq_mama;
	return PCR_OK;
}
// a rule that can drop a product (max_end_mismatch alone tests nothing: its window is empty)
inline bool end3_ruled(const End3Rule &R) { return R.min_clamp3 > 0u || R.window > 0u || R.ident_threshold != 0.0f; }
// 1/length per oligo (optimize.cpp:221, as fill_oligo_planes): what k_item_end3 reads as norm[]
inline std::vector<float> end3_norms(const std::vector<PoolOligo> &ol)
{
	std::vector<float> norm(ol.size());
	for(size_t o = 0;o < ol.size();++o) norm[o] = (float)(1.0/(unsigned)(ol[o].stop - ol[o].start + 1));
	return norm;
}

// k_item_end3 over the items of the shared scratch set, into ctx->pe3_end (enqueued; nothing waits)
int end3_items(pcr_ctx *ctx, SeqSet &S, uint32_t ni, const PoolOligo *d_ol, const float *d_norm, uint32_t window, int use_taq, const ItemEnd *&d_item_end)
{
	int rc;
	if((rc = ctx->pe3_end.ensure(ni)) != PCR_OK) return rc;
	hipLaunchKernelGGL(k_item_end3, dim3((ni + POOL_THREADS - 1)/POOL_THREADS), dim3(POOL_THREADS), 0, ctx->stream, S.db.p, S.db_cap, S.touched.p, S.d_seg_hi,
		(const uint2 *)ctx->shared.items.p, ni, d_ol, d_norm, window, use_taq, (ItemEnd *)ctx->pe3_end.p);
	HIP_TRY(hipGetLastError());
	d_item_end = (const ItemEnd *)ctx->pe3_end.p;
	return PCR_OK;
}

// k_products_join with the rule: one thread per item k, join_walk.  item_tm = NULL: no Tm is read and nothing is floored; item_end =
// NULL: no rule (the plain count).  <false>: count[k], with before != NULL the products past the floor before the rule in
// before[k], and with bits != NULL the bit of every kept product of a pool pair; <true>: records, (begin, end) sort keys and identity
// indices at rec_off[k] ..
template<bool EMIT>
__global__ __launch_bounds__(POOL_THREADS) void k_end3_join(const JoinIn J, const ItemTm *__restrict__ item_tm, float tm_floor,
	const ItemEnd *__restrict__ item_end, const End3Rule R, const uint32_t *__restrict__ intended, const ProductPair *__restrict__ pair_tab,
	uint32_t n_tab, unsigned long long *__restrict__ bits, uint32_t n_pool, uint32_t words, uint32_t *__restrict__ count,
	uint32_t *__restrict__ before, const uint64_t *__restrict__ rec_off, pcr_product_end3 *__restrict__ rec, uint64_t *__restrict__ key,
	uint32_t *__restrict__ ord)
{
	__shared__ int2 ss[POOL_MAX_OLIGOS];
	join_geometry(J, ss);
	const uint32_t k = blockIdx.x*blockDim.x + threadIdx.x;
	if(k >= J.n_items) return;
	const uint2 it = J.items[k];
	const uint32_t g = it.x, x = it.y;
	const uint32_t i = J.touched[g/J.cap]*J.cap + g % J.cap;
	const DevEntry ei = J.db[i];
	uint32_t c = 0, cb = 0;
	uint64_t w = EMIT ? rec_off[k] : 0;
	if(ei.strand == 1){
		ItemTm tp; tp.tm = 0.0f; tp.no_tm = 0;
		if(item_tm) tp = item_tm[k];
		ItemEnd ep; ep.clamp3 = ep.end_mismatch = ep.length = ep.pad = 0; ep.id = 0.0f;
		if(item_end) ep = item_end[k];
		const bool floored = item_tm && tm_floor > 0.0f;
		const bool plus_ok = !item_end || end3_site_ok(ep, R);
		auto keep = [&](uint64_t t, uint32_t y, uint32_t, int32_t p5, int32_t m3, int32_t in_start, int32_t in_len){
			ItemTm tm; tm.tm = 0.0f; tm.no_tm = 0;
			if(item_tm) tm = item_tm[t];
			if(floored && !(((tp.tm < tm.tm) ? tp.tm : tm.tm) >= tm_floor)) return;   // min(tm_plus, tm_minus) >= tm_floor
			++cb;
			ItemEnd em; em.clamp3 = em.end_mismatch = em.length = em.pad = 0; em.id = 0.0f;
			if(item_end && !end3_product_ok(item_end, R, plus_ok, ep, t, em)) return;
			if(EMIT){
				pcr_product_end3 r;
				r.plus_oligo = x; r.minus_oligo = y; r.sequence = ei.seq; r.begin = p5; r.end = m3;
				r.inner_start = in_start; r.inner_length = in_len; r.intended = 0;
				r.tm_plus = tp.tm; r.tm_minus = tm.tm;
				r.flags = (tp.no_tm ? PCR_PRODUCT_PLUS_NO_TM : 0u) | (tm.no_tm ? PCR_PRODUCT_MINUS_NO_TM : 0u);
				r.reserved = 0;
				r.clamp3_plus = ep.clamp3; r.clamp3_minus = em.clamp3;
				r.end_mismatch_plus = ep.end_mismatch; r.end_mismatch_minus = em.end_mismatch;
				r.id_plus = ep.id; r.id_minus = em.id;
				r.reserved2 = 0;
				rec[w] = r;
				key[w] = product_key1(p5, m3);
				ord[w] = (uint32_t)w;
				++w;
			}
			else{
				++c;
				const uint32_t b = x*J.n_ol + y;
				if(bits && ((intended[b >> 5] >> (b & 31)) & 1u)){
					uint32_t lo = 0, above = n_tab;                                  // pair_tab[lo].key <= b < pair_tab[above].key; an intended b is in the table
					while(above - lo > 1u){
						const uint32_t mid = lo + (above - lo)/2u;
						if(pair_tab[mid].key <= b) lo = mid; else above = mid;
					}
					const ProductPair pp = pair_tab[lo];
					if(pp.key == b){
						const unsigned long long bit = 1ull << (ei.seq & 63u);
						const size_t word = ei.seq >> 6;
						if(pp.fr_row != PTM_NO_ROW) atomicOr(bits + (size_t)pp.fr_row*words + word, bit);
						if(pp.rf_row != PTM_NO_ROW) atomicOr(bits + ((size_t)n_pool + pp.rf_row)*words + word, bit);
					}
				}
			}
		};
		// (a plus site below the floor keeps no product; one that fails the rule keeps none either, but its products count before the rule)
		const bool count_before = !EMIT && before != nullptr;
		if(!(floored && tp.tm < tm_floor) && (plus_ok || count_before)) join_walk<false>(J, ss, g, x, i, ei, 0u, keep);
	}
	if(!EMIT){
		count[k] = c;
		if(before) before[k] = cb;
	}
}

} // namespace

extern "C" {

int64_t pcr_pool_products_end3(pcr_ctx *ctx, pcr_set which, const pcr_pair *pool, uint32_t n_pool, float threshold,
	int32_t amp_min, int32_t amp_max, const pcr_thermo_args *args, float template_strand, float tm_floor,
	const pcr_end3_rule *rule, uint32_t *oligo_id, pcr_product_end3 *out, uint64_t cap,
	uint64_t *bits_fr, uint64_t *bits_rf, uint64_t *n_before_rule)
{
	static_assert(sizeof(pcr_product_end3) == 64, "record layout");
	static_assert(offsetof(pcr_product_end3, clamp3_plus) == sizeof(pcr_product_tm), "the first 48 bytes are pcr_product_tm");
	static_assert(sizeof(ItemEnd) == sizeof(uint2), "table layout");
	// ---- the arguments, before the handle (pcr_pool_products_tm's checks in its order; without args no concentration or salt is looked at)
	if(!set_ok(which)){ g_err = "pcr_pool_products_end3: unknown sequence set"; return PCR_ERR_ARG; }
	if(which != PCR_SET_TARGET && which != PCR_SET_BACKGROUND){ g_err = "pcr_pool_products_end3: PCR_SET_MULTIPLEX is not supported (PCR_SET_TARGET or PCR_SET_BACKGROUND)"; return PCR_ERR_ARG; }
	if((n_pool && (!pool || !oligo_id)) || (cap && !out)){ g_err = "pcr_pool_products_end3: bad argument"; return PCR_ERR_ARG; }
	if(n_pool > PCR_POOL_MAX_PAIRS){ g_err = "pcr_pool_products_end3: pool larger than PCR_POOL_MAX_PAIRS"; return PCR_ERR_ARG; }
	if(args){
		if(!(template_strand >= 0.0f) || !(args->primer_strand >= 0.0f)){ g_err = "pcr_pool_products_end3: negative strand concentration (NucCruc::strand, nuc_cruc.h:818-826)"; return PCR_ERR_ARG; }
		if(!(args->salt >= 1.0e-6f && args->salt <= 1.0f)){ g_err = "pcr_pool_products_end3: salt outside [1e-6, 1] (NucCruc::salt, nuc_cruc.h:780-788)"; return PCR_ERR_ARG; }
	}
	std::vector<PoolOligo> ol;
	std::vector<SiteOligoX> olx;
	if(site_oligo_table("pcr_pool_products_end3", "an oligo", "primer_strand", pool, n_pool, threshold, args, template_strand, oligo_id, ol, olx) != PCR_OK) return PCR_ERR_ARG;
	if(!std::isfinite(tm_floor)){ g_err = "pcr_pool_products_end3: tm_floor is not finite"; return PCR_ERR_ARG; }
	End3Rule R;
	int use_taq;
	if(end3_rule_of("pcr_pool_products_end3", rule, R, use_taq) != PCR_OK) return PCR_ERR_ARG;
	if(!args && tm_floor > 0.0f){ g_err = "pcr_pool_products_end3: tm_floor > 0 without args (no thermodynamics to floor)"; return PCR_ERR_ARG; }
	if(!ctx){ g_err = "pcr_pool_products_end3: null handle"; return PCR_ERR_ARG; }
	{ const int drc = drain(ctx); if(drc != PCR_OK) return drc; }
	HIP_TRY(hipSetDevice(ctx->device));
	SeqSet &S = ctx->sets[which];
	if(!S.have_db){ g_err = "pcr_pool_products_end3: no word DB (call pcr_select_words or pcr_select_sites first)"; return PCR_ERR_STATE; }
	if(n_before_rule) *n_before_rule = 0;
	if(n_pool == 0) return 0;
	const uint32_t words = (uint32_t)((S.n + 63)/64);
	const size_t row_words = (size_t)n_pool*words;
	const bool want_bits = bits_fr || bits_rf;
	// whatever the count, the rows asked for are written in full
	auto zero_rows = [&](){
		if(bits_fr) memset(bits_fr, 0, row_words*sizeof(uint64_t));
		if(bits_rf) memset(bits_rf, 0, row_words*sizeof(uint64_t));
	};
	{ const int erc = ensure_touched(ctx, S); if(erc != PCR_OK) return erc; }
	if(S.n_entries == 0 || S.n_touched == 0){ zero_rows(); return 0; }
	const uint32_t n_ol = (uint32_t)ol.size();
	const bool melt = args && (tm_floor > 0.0f || cap > 0 || want_bits);         // pcr_pool_products_tm's condition
	const bool ruled = end3_ruled(R);
	const bool ends = ruled || cap > 0;                                          // else: nothing reads an ItemEnd
	// the intended bitmap and the rows of the first pool pair per (plus, minus): pcr_pool_products_tm's (PairTable); then 1/length per oligo
	PairTable pair_rows(oligo_id, n_pool, n_ol);
	const std::vector<uint32_t> &intended = pair_rows.intended;
	const std::vector<ProductPair> &tab = pair_rows.tab;
	const std::vector<float> norm = end3_norms(ol);
	int rc;
	const size_t ol_bytes = ol.size()*sizeof(PoolOligo), tab_bytes = tab.size()*sizeof(ProductPair), olx_bytes = olx.size()*sizeof(SiteOligoX),
		int_bytes = intended.size()*sizeof(uint32_t), norm_bytes = norm.size()*sizeof(float);
	std::vector<uint8_t> blob(ol_bytes + tab_bytes + olx_bytes + int_bytes + norm_bytes);   // 32-, 16-, 8-, 4- and 4-byte records, in that order: each is aligned
	memcpy(blob.data(), ol.data(), ol_bytes);
	memcpy(blob.data() + ol_bytes, tab.data(), tab_bytes);
	memcpy(blob.data() + ol_bytes + tab_bytes, olx.data(), olx_bytes);
	memcpy(blob.data() + ol_bytes + tab_bytes + olx_bytes, intended.data(), int_bytes);
	memcpy(blob.data() + ol_bytes + tab_bytes + olx_bytes + int_bytes, norm.data(), norm_bytes);
	ItemScratch &X = ctx->shared;
	const ItemBufs B = X.bufs();
	if((rc = X.in.ensure(blob.size())) != PCR_OK) return rc;
	const PoolOligo *d_ol = (const PoolOligo *)X.in.p;
	const ProductPair *d_tab = (const ProductPair *)(X.in.p + ol_bytes);
	const SiteOligoX *d_olx = (const SiteOligoX *)(X.in.p + ol_bytes + tab_bytes);
	const uint32_t *d_intended = (const uint32_t *)(X.in.p + ol_bytes + tab_bytes + olx_bytes);
	const float *d_norm = (const float *)(X.in.p + ol_bytes + tab_bytes + olx_bytes + int_bytes);
	HIP_TRY(hipMemcpyAsync(X.in.p, blob.data(), blob.size(), hipMemcpyHostToDevice, ctx->stream));
	// ---- 1. the items (item_count waits: blob is read by then)
	uint64_t n_items = 0;
	if((rc = item_count(ctx, S, d_ol, n_ol, B, n_items)) != PCR_OK) return rc;
	if(n_items >= POOL_MAX_ITEMS){ g_err = "pcr_pool_products_end3: too many (entry, oligo) hits"; return PCR_ERR_CAPACITY; }
	if(n_items == 0){ zero_rows(); return 0; }
	if((rc = item_fill(ctx, S, d_ol, n_ol, B, n_items)) != PCR_OK) return rc;
	const uint32_t ni = (uint32_t)n_items;
	const unsigned grid_i = (ni + POOL_THREADS - 1)/POOL_THREADS;
	if((rc = X.cnt.ensure((size_t)ni + 1)) != PCR_OK) return rc;                // (the entry counts are spent)
	// ---- 2. the 3' end per item
	const ItemEnd *d_item_end = nullptr;
	if(ends && (rc = end3_items(ctx, S, ni, d_ol, d_norm, R.window, use_taq, d_item_end)) != PCR_OK) return rc;
	// ---- 3. job offsets, the jobs, Tm per item
	if(melt && (rc = melt_items("pcr_pool_products_end3", ctx, S, d_ol, d_olx, ni, args->salt, B)) != PCR_OK) return rc;
	const ItemTm *d_item_tm = melt ? (const ItemTm *)X.item_tm.p : nullptr;
	// ---- 4. the join: count (and the bits), the before-rule sum, scan
	unsigned long long *d_bits = nullptr;
	if(want_bits){
		if((rc = ctx->pe3_bits.ensure(2*row_words)) != PCR_OK) return rc;
		HIP_TRY(hipMemsetAsync(ctx->pe3_bits.p, 0, 2*row_words*sizeof(uint64_t), ctx->stream));
		d_bits = (unsigned long long *)ctx->pe3_bits.p;
	}
	const bool sum_before = n_before_rule && ruled;                              // (without a rule it is the count)
	size_t red_bytes = 0;
	if(sum_before){
		if((rc = ctx->pe3_before.ensure(ni)) != PCR_OK) return rc;
		if((rc = ctx->pe3_sum.ensure(1)) != PCR_OK) return rc;
		HIP_TRY(rocprim::reduce(nullptr, red_bytes, rocprim::make_transform_iterator((const uint32_t *)ctx->pe3_before.p, End3Widen()), ctx->pe3_sum.p,
			uint64_t(0), ni, rocprim::plus<uint64_t>(), ctx->stream));
		if((rc = ctx->pe3_tmp.ensure(red_bytes + 16)) != PCR_OK) return rc;
	}
	const JoinIn J{S.db.p, S.db_cap, S.touched.p, S.d_seg_hi, X.items.p, ni, X.eoff.p, d_ol, n_ol, S.planes.p, S.d_blk_off.p, S.d_len.p,
		S.d_has_eos.p, amp_min, amp_max};
	hipLaunchKernelGGL(k_end3_join<false>, dim3(grid_i), dim3(POOL_THREADS), 0, ctx->stream, J, d_item_tm, tm_floor, d_item_end, R, d_intended, d_tab,
		(uint32_t)tab.size(), d_bits, n_pool, words, X.cnt.p, sum_before ? ctx->pe3_before.p : (uint32_t *)nullptr, (const uint64_t *)nullptr,
		(pcr_product_end3 *)nullptr, (uint64_t *)nullptr, (uint32_t *)nullptr);
	HIP_TRY(hipGetLastError());
	if(sum_before) HIP_TRY(rocprim::reduce(ctx->pe3_tmp.p, red_bytes, rocprim::make_transform_iterator((const uint32_t *)ctx->pe3_before.p, End3Widen()),
		ctx->pe3_sum.p, uint64_t(0), ni, rocprim::plus<uint64_t>(), ctx->stream));
	uint64_t total = 0, total_before = 0;
	uint32_t bad = 0;                                                            // (without a melt no k_item_tm ran: the flag is another call's)
	if((rc = scan_total(ctx, X.cnt.p, X.ioff, X.tmp, ni, total, [&]() -> int {
		if(melt) HIP_TRY(hipMemcpyAsync(&bad, X.flag.p, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
		if(sum_before) HIP_TRY(hipMemcpyAsync(&total_before, ctx->pe3_sum.p, sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
		if(bits_fr) HIP_TRY(hipMemcpyAsync(bits_fr, ctx->pe3_bits.p, row_words*sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
		if(bits_rf) HIP_TRY(hipMemcpyAsync(bits_rf, ctx->pe3_bits.p + row_words, row_words*sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
		return PCR_OK;
	})) != PCR_OK) return rc;
	if(bad & 1u){ g_err = "pcr_pool_products_end3: internal trace-back error"; return PCR_ERR_RANGE; }
	if(!sum_before) total_before = total;
	pair_rows.copy_repeated_rows(oligo_id, n_pool, words, bits_fr, bits_rf);
	if(total >= POOL_MAX_ITEMS || total_before >= POOL_MAX_ITEMS){ g_err = "pcr_pool_products_end3: too many products"; return PCR_ERR_CAPACITY; }
	if(n_before_rule) *n_before_rule = total_before;
	if(total == 0 || total > cap) return (int64_t)total;                         // count only: out is left as it is
	// ---- 4'. emit at the scanned offsets; 5. the key order
	const uint32_t nr = (uint32_t)total;
	if((rc = ctx->pe3_rec.ensure(2*(size_t)nr)) != PCR_OK) return rc;
	if((rc = ctx->pe3_keys.ensure(2*(size_t)nr)) != PCR_OK) return rc;
	if((rc = ctx->pe3_ord.ensure(2*(size_t)nr)) != PCR_OK) return rc;
	pcr_product_end3 *r0 = ctx->pe3_rec.p, *r1 = r0 + nr;
	hipLaunchKernelGGL(k_end3_join<true>, dim3(grid_i), dim3(POOL_THREADS), 0, ctx->stream, J, d_item_tm, tm_floor, d_item_end, R, d_intended, d_tab,
		(uint32_t)tab.size(), (unsigned long long *)nullptr, n_pool, words, (uint32_t *)nullptr, (uint32_t *)nullptr, (const uint64_t *)X.ioff.p,
		r0, ctx->pe3_keys.p, ctx->pe3_ord.p);
	HIP_TRY(hipGetLastError());
	if((rc = product_order(ctx, r0, ctx->pe3_keys.p, ctx->pe3_ord.p, nr, pool_bits(S.n), pool_bits(n_ol), d_intended, n_ol, X.tmp)) != PCR_OK) return rc;
	HIP_TRY(hipMemcpyAsync(out, r1, (size_t)nr*sizeof(pcr_product_end3), hipMemcpyDeviceToHost, ctx->stream));
	HIP_TRY(hipStreamSynchronize(ctx->stream));
	return (int64_t)total;
}

} // extern "C"
