namespace {

// The lists a pass's planners make and its launches read (plan_seed2, plan_seed3_slices, plan_seed1).  They belong to the pass
// (PassJob), not to the handle: the caller's thread may plan the next pass while the launcher thread still reads this one's.
struct PlanLists : pcrseed::SeedLists {
	// second form of the seed scan: the lists of pcrseed::SeedLists (pcr_seed_lists.hpp) and the floors
	std::vector<uint8_t> s2_floors;
	std::vector<pcr_ctx::S3Launch> s3_launch;      // third form: per launch group, the workgroups' slices of the chunk list
	std::vector<uint32_t> s1_seeds;                // first form, tables built on the device: the pass's seed list
	void clear()
	{
		s2_seeds.clear(); s2_masks.clear(); s2_floors.clear(); s2_group_end.clear(); s2_group_offmask.clear(); s2_group_or.clear(); s2_group_nor.clear();
		s3_launch.clear(); s3_prefix.clear(); s3_spans.clear(); s1_seeds.clear();
	}
};

// The seeds of a pass for the second form of the seed scan: per orientation from the cache (derived on a miss), listed as
// code << 14 | slot offset << 9 | orientation WITHIN ITS GROUP, in groups of at most S2_MAX_OR whole orientations, each of which
// fits the LDS budget of one launch.  One launch per group: IUPAC primers expand to more 9-gram seeds than one launch holds
// (two launches of this form still beat the first form, 2 x ~65 vs 178 + 22 us at C5's shard), and the reference's default
// batch of 1 000 trial assays (pcramp.h:32) is 4 000 orientations = 16+ groups (r02 sent it to the first form with host-built
// tables: 21 ms per select_words on a C5 shard).  false: an orientation whose seeds alone exceed one launch.
constexpr uint32_t S2_MAX_GROUPS = 4096;
// S3 (optional): the set whose position index the third form will read.  The seeds are then the oligo's FOLDED seeds, from a cache
// of their own (ctx->seed_lists.third; PCRAMP_S3_NEXT=0: the plain 9-gram list with span A..T), listed in the same u32 form with a
// span byte per seed beside them (L.s3_spans), and the chunk list of every launch group (L.s3_prefix: the running number of
// 64-entry chunks of the group's seeds' spans, its total behind it) is made alongside, from chunk counts cached beside each
// oligo's seeds for the sets last used.  The listing itself is plain C++: pcrseed::list_seeds (pcr_seed_lists.hpp).
static_assert(sizeof(pcrseed::Mask16) == sizeof(uint4) && alignof(pcrseed::Mask16) <= alignof(uint4), "the mask entry is the device's uint4");
static_assert(offsetof(pcrseed::Mask16, y) == offsetof(uint4, y) && offsetof(pcrseed::Mask16, w) == offsetof(uint4, w), "the mask entry is the device's uint4");
static_assert(S2_Q == 9, "pcrseed::derive lists 9-gram seeds");
static_assert(pcrseed::CHUNK_SETS == pcr_ctx::S3_CHUNK_SETS, "generations kept per cache entry");
bool plan_seed2(pcr_ctx *ctx, PlanLists &L, const std::vector<pcrhost::Candidate> &cand, std::vector<uint32_t> &or_seed, std::vector<uint32_t> &or_plain, uint32_t &irr_off_mask,
	const SeqSet *S3 = nullptr)
{
	// the tables of a launch must fit one CU's LDS; the third form keeps only the masks and a slice of the lists there: more orientations
	// (9-bit ids) and as many seeds as the pass has -- plan_seed3_slices() checks its LDS need afterwards
	const pcrseed::Limits lim2 = { S2_MAX_OR, S2_MAX_SEEDS, sizeof(S2Shared) + 1024, 160*1024, S2_MAX_GROUPS };
	const pcrseed::Limits lim3 = { S3_MAX_OR, S3_MAX_SEEDS, 0, ~size_t(0), S2_MAX_GROUPS };
	pcrseed::SetIndex ix = { nullptr, 0 };
	if(S3){ ix.start = S3->pix_start_h.data(); ix.generation = S3->pix_generation; }
	return pcrseed::list_seeds(ctx->seed_lists, S3 ? lim3 : lim2, cand.data(), cand.size(), S3 ? &ix : nullptr, ctx->s3_next, L, or_seed, or_plain, irr_off_mask);
}

// Third form: the chunks of every launch group dealt to G workgroups in equal contiguous shares, and per workgroup the first seed of its
// share (pcrseed::plan_slices: a merge walk over the group's chunk list).  false: some group's largest slice does not fit the LDS (many
// seeds whose runs are empty side by side: tiny target sets) -- the caller plans again within the second form's limits.
constexpr size_t S3_LDS_BUDGET = 120*1024;
// 1024-thread workgroups, two per CU (512 threads x 4 per CU: within the spread of the repeated default, profiles/dbg/r03_ab_s3_grid.txt)
constexpr uint32_t S3_WG_THREADS = 1024;
uint32_t seed3_grid(const pcr_ctx *ctx) { return std::min<uint32_t>(2*ctx->n_cu, S3_MAX_WG); }
bool plan_seed3_slices(pcr_ctx *ctx, PlanLists &PL, bool with_irr)
{
	return pcrseed::plan_slices(PL, PL.s3_launch, seed3_grid(ctx), 16u*(S3_WG_THREADS/64), S3_MAX_WG, S3_LDS_BUDGET, with_irr);
}

// The seeds of a pass for the first form with device-built tables: per orientation from the cache (8-gram seeds), listed as
// code | slot offset << 16 | orientation << 21.  When the lists exceed S1_MAX_SEEDS (low thresholds: hundreds of codes per
// orientation) the orientations with the longest lists go to the bit-sliced scan.
void plan_seed1(pcr_ctx *ctx, PlanLists &L, const std::vector<pcrhost::Candidate> &cand, std::vector<uint32_t> &or_seed, std::vector<uint32_t> &or_plain, uint32_t &irr_off_mask)
{
	const uint32_t n_or = 2*(uint32_t)cand.size();
	std::vector<uint32_t> &out = L.s1_seeds;
	out.clear();
	irr_off_mask = 0;
	if(ctx->s1_cache.size() > 16384) ctx->s1_cache.clear();
	std::vector<const pcr_ctx::S2Entry *> ent(n_or);
	size_t total = 0;
	for(uint32_t o = 0;o < n_or;++o){
		const pcrhost::Candidate &c = cand[o >> 1];
		const Planes &m = (o & 1u) ? c.rc : c.fwd;
		const pcr_ctx::S2Key key = {m.a, m.c, m.g, m.t, c.floor_};
		auto it = ctx->s1_cache.find(key);
		if(it == ctx->s1_cache.end()){
			pcr_ctx::S2Entry e; e.off_mask = 0;
			ctx->s2_tmp.clear();
			e.seedable = pcrhost::orientation_seeds(m, c.floor_, 0, ctx->s2_tmp);
			e.seeds.reserve(ctx->s2_tmp.size());
			for(const pcrhost::Seed &sd : ctx->s2_tmp){ e.seeds.push_back(sd.code | ((uint32_t)sd.off << 16)); e.off_mask |= 1u << sd.off; }
			it = ctx->s1_cache.emplace(key, std::move(e)).first;
		}
		ent[o] = &it->second;                                            // (unordered_map: references stay valid across insertions)
		if(ent[o]->seedable) total += ent[o]->seeds.size();
	}
	std::vector<uint8_t> drop(n_or, 0);
	if(total > S1_MAX_SEEDS){
		std::vector<uint32_t> by_len;
		for(uint32_t o = 0;o < n_or;++o){ if(ent[o]->seedable) by_len.push_back(o); }
		std::stable_sort(by_len.begin(), by_len.end(), [&](uint32_t x, uint32_t y){ return ent[x]->seeds.size() > ent[y]->seeds.size(); });
		for(size_t i = 0;i < by_len.size() && total > S1_MAX_SEEDS;++i){ drop[by_len[i]] = 1; total -= ent[by_len[i]]->seeds.size(); }
	}
	out.resize(total);
	size_t at = 0;
	for(uint32_t o = 0;o < n_or;++o){
		const pcr_ctx::S2Entry &e = *ent[o];
		if(!e.seedable || drop[o]){ or_plain.push_back(o); continue; }
		or_seed.push_back(o);
		const uint32_t tag = o << 21;
		for(size_t k = 0;k < e.seeds.size();++k) out[at + k] = e.seeds[k] | tag;
		at += e.seeds.size();
		if(!(o & 1u)) irr_off_mask |= e.off_mask;                       // slot offsets at which forward seeds sit (irregular-word scan)
	}
}

// The first form's plan when its tables are built on the HOST (passes with 5'/3' shift candidates, more than S1_MAX_OR
// orientations, PCRAMP_SEED_TABLES=host): seeds per orientation (shift candidates inherit the unshifted oligo's), then the
// tables of pcr_scan_seed.inc: presence bitmap + rank (the LDS image), one head word per distinct code, grouped seed lists
// of the codes shared by several seeds.  Too many distinct codes, or a code shared by more than 255 seeds, sends the densest
// quarter of the orientations (with shift candidates: everything) to the bit-sliced path.
struct HostSeedPlan {
	std::vector<pcrhost::Seed> seeds;
	std::vector<std::vector<std::pair<uint16_t, int8_t> > > inheritors;   // per orientation: (shifted orientation, shift) sharing its seeds
	size_t n_inherited = 0;
	std::vector<uint32_t> image, heads, multi;
};

int plan_seed_host(pcr_ctx *ctx, const std::vector<pcrhost::Candidate> &cand, HostSeedPlan &H, std::vector<uint32_t> &or_seed, std::vector<uint32_t> &or_plain,
	uint32_t &irr_off_mask)
{
	const uint32_t n_or = 2*(uint32_t)cand.size();
	struct OrientInfo { uint32_t begin, end; int max_exact_pos; bool seeded; };
	std::vector<OrientInfo> info;
	std::vector<pcrhost::Seed> &seeds = H.seeds;
	std::vector<std::vector<std::pair<uint16_t, int8_t> > > &inheritors = H.inheritors;
	size_t &n_inherited = H.n_inherited;
	std::vector<uint32_t> &image = H.image, &heads = H.heads, &multi = H.multi;
	// a 5'/3' shift candidate inherits the seeds of the unshifted oligo, moved by its shift, as long as no
	// padded 8-window would have to be clamped at the end of the word (it costs 1/10 of deriving them anew)
	info.assign(n_or, OrientInfo());
	inheritors.assign(n_or, std::vector<std::pair<uint16_t, int8_t> >());
	seeds.reserve((size_t)n_or*32);
	for(uint32_t o = 0;o < n_or;++o){
		const pcrhost::Candidate &c = cand[o >> 1];
		OrientInfo &me = info[o];
		me.begin = (uint32_t)seeds.size(); me.max_exact_pos = -1;
		const uint32_t bo = 2*c.base + (o & 1u);
		const int32_t sh = (o & 1u) ? -c.shift : c.shift;
		if(c.base != (o >> 1) && info[bo].seeded && info[bo].max_exact_pos <= 24 && info[bo].max_exact_pos + sh <= 24){
			inheritors[bo].push_back(std::make_pair((uint16_t)o, (int8_t)sh));   // its seeds = those of bo with off + sh: expanded when the table is built
			n_inherited += info[bo].end - info[bo].begin;
			me.seeded = true; me.max_exact_pos = (info[bo].max_exact_pos < 0) ? -1 : info[bo].max_exact_pos + sh;
		}
		else me.seeded = pcrhost::orientation_seeds((o & 1) ? c.rc : c.fwd, c.floor_, o, seeds, &me.max_exact_pos);
		me.end = (uint32_t)seeds.size();
		if(me.seeded) or_seed.push_back(o); else or_plain.push_back(o);
	}
	if(or_seed.empty()) return PCR_OK;
	// count[] / own[] (one entry per 8-gram code) are kept all-zero between passes: only the entries a pass touched
	// are cleared again (two 64K-entry memsets per pass were ~8 us of the host plan)
	if(ctx->seed_count.size() != 65536){ ctx->seed_count.assign(65536, 0); ctx->seed_own.assign(65536, 0); }
	std::vector<uint16_t> &count = ctx->seed_count;
	bool overflow = false;
	uint32_t distinct = 0;
	std::vector<uint8_t> &own = ctx->seed_own;                          // seeds listed under the code (its inheritors come on top)
	for(;;){
		image.assign(SEED_IMAGE_WORDS, 0u);
		overflow = false; distinct = 0;
		for(const pcrhost::Seed &sd : seeds){
			uint16_t &c = count[sd.code];
			if(c == 0){ image[sd.code >> 5] |= 1u << (sd.code & 31); ++distinct; }
			c = (uint16_t)(c + 1 + (inheritors.empty() ? 0 : inheritors[sd.orient].size()));
			if(c > 255){ overflow = true; break; }
			++own[sd.code];
		}
		if(distinct > SEED_MAX_DISTINCT) overflow = true;
		if(!overflow || n_inherited || or_seed.size() < 2) break;
		// Too dense (low thresholds: hundreds of codes per orientation): hand the quarter of the seeded orientations
		// with the longest code lists to the bit-sliced scan and count again.
		for(const pcrhost::Seed &sd : seeds){ count[sd.code] = 0; own[sd.code] = 0; }
		std::vector<uint32_t> by_len(or_seed);
		std::stable_sort(by_len.begin(), by_len.end(), [&](uint32_t x, uint32_t y){ return info[x].end - info[x].begin > info[y].end - info[y].begin; });
		const size_t n_drop = (by_len.size() + 3)/4;
		std::vector<uint8_t> drop(n_or, 0);
		for(size_t i = 0;i < n_drop;++i) drop[by_len[i]] = 1;
		std::vector<pcrhost::Seed> kept; kept.reserve(seeds.size());
		for(uint32_t o = 0;o < n_or;++o){
			const uint32_t b = info[o].begin, e = info[o].end;
			info[o].begin = (uint32_t)kept.size();
			if(!drop[o]) kept.insert(kept.end(), seeds.begin() + b, seeds.begin() + e);
			info[o].end = (uint32_t)kept.size();
			if(drop[o]) info[o].seeded = false;
		}
		seeds.swap(kept);
		or_seed.clear(); or_plain.clear();
		for(uint32_t o = 0;o < n_or;++o){ if(info[o].seeded) or_seed.push_back(o); else or_plain.push_back(o); }
	}
	for(const pcrhost::Seed &sd : seeds){                                 // slot offsets at which forward seeds sit (irregular-word scan)
		if(sd.orient & 1u) continue;
		irr_off_mask |= 1u << sd.off;
		if(!inheritors.empty()){ for(const std::pair<uint16_t, int8_t> &in : inheritors[sd.orient]) irr_off_mask |= 1u << (sd.off + in.second); }
	}
	if(overflow){
		or_plain.clear(); or_seed.clear(); image.clear();
		for(uint32_t o = 0;o < n_or;++o) or_plain.push_back(o);
	}
	else{
		uint16_t *rank16 = (uint16_t *)(image.data() + SEED_BITMAP_WORDS);
		uint32_t run = 0;
		for(uint32_t w = 0;w < SEED_BITMAP_WORDS;++w){ rank16[w] = (uint16_t)run; run += (uint32_t)__builtin_popcount(image[w]); }
		heads.assign(distinct, 0u);
		// first pass: reserve the multi ranges (head = start << 8 | filled so far); second: fill
		uint32_t n_multi = 0;
		for(const pcrhost::Seed &sd : seeds){
			const uint32_t h = rank16[sd.code >> 5] + (uint32_t)__builtin_popcount(image[sd.code >> 5] & ((1u << (sd.code & 31)) - 1u));
			if(count[sd.code] == 1){ heads[h] = SEED_SINGLE | ((uint32_t)sd.orient << 8) | sd.off; continue; }
			if(heads[h] == 0){ heads[h] = 0x40000000u | n_multi; n_multi += own[sd.code]; }   // bit 30: range reserved, low bits = start
		}
		std::vector<uint32_t> raw(n_multi, 0u);                  // per code, in generation order: orient | off << 24
		std::vector<uint8_t> &fill = ctx->seed_fill; fill.assign(distinct, 0);
		for(const pcrhost::Seed &sd : seeds){
			if(count[sd.code] == 1) continue;
			const uint32_t h = rank16[sd.code >> 5] + (uint32_t)__builtin_popcount(image[sd.code >> 5] & ((1u << (sd.code & 31)) - 1u));
			const uint32_t start = heads[h] & 0x3FFFFFFFu;
			raw[start + fill[h]++] = (uint32_t)sd.orient | ((uint32_t)sd.off << 24);
		}
		// Group the seeds of a code: slot shifts of one oligo orientation (consecutive candidates, so consecutive
		// here) whose base-aligned offset boff = off - shift is the same lie over the same target bases; their
		// match count is taken once, with the unshifted orientation at window x - boff (layout: pcr_scan_seed.inc).
		multi.clear(); multi.reserve(n_multi + n_multi/2 + 16);
		for(uint32_t h = 0;h < distinct;++h){
			if(heads[h] & SEED_SINGLE) continue;
			const uint32_t start = heads[h] & 0x3FFFFFFFu, n = fill[h];
			const uint32_t out0 = (uint32_t)multi.size();
			uint32_t header_at = 0, members = 0, cur_base = 0xFFFFFFFFu; int32_t cur_boff = -1;
			for(uint32_t e = 0;e < n;++e){
				const uint32_t sd = raw[start + e], orient = sd & 0xFFFFu, off = sd >> 24;
				const pcrhost::Candidate &c = cand[orient >> 1];
				const int32_t sh = (orient & 1u) ? -c.shift : c.shift;
				int32_t boff = (int32_t)off - sh;
				uint32_t base_orient = 2*c.base + (orient & 1u);
				if(boff < 0 || boff > 24){ boff = (int32_t)off; base_orient = orient; }   // the unshifted window would leave the word: stands alone
				if(members && base_orient == cur_base && boff == cur_boff && members < 256){
					multi.push_back(sd); ++members;
					multi[header_at] = SEED_GROUP | cur_base | ((uint32_t)cur_boff << 16) | ((members - 1) << 21);
				}
				else{
					header_at = (uint32_t)multi.size(); members = 1; cur_base = base_orient; cur_boff = boff;
					multi.push_back(SEED_GROUP | cur_base | ((uint32_t)cur_boff << 16));
					multi.push_back(sd);
				}
				// the shift candidates that inherit this seed: same target bases, off moved by their shift
				if(!inheritors.empty()){
					for(const std::pair<uint16_t, int8_t> &in : inheritors[orient]){
						if(members == 256){        // header field full: open another group with the same leader
							header_at = (uint32_t)multi.size(); members = 0;
							multi.push_back(SEED_GROUP | cur_base | ((uint32_t)cur_boff << 16));
						}
						multi.push_back((uint32_t)in.first | ((uint32_t)((int32_t)off + in.second) << 24)); ++members;
						multi[header_at] = SEED_GROUP | cur_base | ((uint32_t)cur_boff << 16) | ((members - 1) << 21);
					}
				}
			}
			heads[h] = (out0 << 9) | ((uint32_t)multi.size() - out0);
		}
		n_multi = (uint32_t)multi.size();
		if(n_multi >= (1u << 22)){ ctx->seed_count.clear(); g_err = "pcr_select_words: seed table too large"; return PCR_ERR_CAPACITY; }
	}
	return PCR_OK;
}

// ---- The select pass proper, in the order it runs: plan (which scan form takes the seeded orientations), stage (the tables
// to the device), launch (one function per form), tail (fused k_post, or k_touched / k_finalize / k_publish).

enum class ScanForm { Popcount, BitSliced, Seed1Host, Seed1Dev, Seed2, Seed3 };
inline const char *form_name(ScanForm f)
{
	static const char *const names[] = { "popcount", "bitsliced", "seed1-host", "seed1-dev", "seed2", "seed3" };
	return names[(int)f];
}
inline bool is_seed1(ScanForm f) { return f == ScanForm::Seed1Host || f == ScanForm::Seed1Dev; }
inline bool is_seed2(ScanForm f) { return f == ScanForm::Seed2 || f == ScanForm::Seed3; }   // (the third form runs on the second's plan and tables)

struct ScanPlan {
	ScanForm form = ScanForm::BitSliced;              // the scan that serves the seeded orientations; BitSliced: the plan seeds none
	std::vector<uint32_t> or_seed, or_plain;          // orientation ids
	uint32_t irr_off_mask = 0;
	HostSeedPlan H;                                   // Seed1Host only
	bool s3_with_irr = false;                         // Seed3: the set has live irregular words, which that form looks up through their index
	bool need_plain = false, need_seedset = false;    // bit-sliced tables: unseedable orientations (all tiles) / seedable ones (IUPAC tiles)
	size_t n_seeds = 0;                               // of the form that planned the pass (debug line)
	uint32_t n_live = 0, min_len = 0;                 // irregular words whose size counter reaches min_oligo_length; that length
	void reset()                                      // (the vectors keep their storage: a recycled PassJob allocates nothing)
	{
		form = ScanForm::BitSliced; or_seed.clear(); or_plain.clear(); irr_off_mask = 0;
		H.seeds.clear(); H.inheritors.clear(); H.n_inherited = 0; H.image.clear(); H.heads.clear(); H.multi.clear();
		s3_with_irr = need_plain = need_seedset = false; n_seeds = 0; n_live = min_len = 0;
	}
};

inline uint32_t live_irregular(const SeqSet &S, uint32_t min_oligo_length)
{
	uint32_t n_live = 0;
	for(uint32_t k = std::min<uint32_t>(min_oligo_length, 256);k < 256;++k) n_live += S.irr_size_count[k];
	return n_live;
}

// Can the irregular words come in through their index?  No word of the set holds IUPAC slots, the index counts its entries in
// 32 bits (24 per word), and no key is shared by more words than a wave should walk (ensure_irr_index, built on first use).
int irr_index_usable(pcr_ctx *ctx, SeqSet &S, bool &usable)
{
	usable = false;
	if(S.irr_n_multi != 0 || (uint64_t)24*S.n_irr >= (uint64_t(1) << 32)) return PCR_OK;
	const int rc = ensure_irr_index(ctx, S);
	usable = rc == PCR_OK && S.irx_usable;
	return rc;
}

// Scan plan.  version 3 (default): orientations that can be seeded go through the pigeonhole seed scan; the others, and every
// tile holding IUPAC target codes, through the bit-sliced counter.  version 2: bit-sliced counter for everything.  version 1:
// one popcount per (window, orientation).  The planners fill the pass's lists (PlanLists L), which the launches read.
int choose_scan_form(pcr_ctx *ctx, SeqSet &S, const std::vector<pcrhost::Candidate> &cand, int optimize_5, int optimize_3, uint32_t min_oligo_length, ScanPlan &P, PlanLists &L)
{
	const uint32_t n_or = 2*(uint32_t)cand.size();
	std::vector<uint32_t> &or_seed = P.or_seed, &or_plain = P.or_plain;
	P.min_len = min_oligo_length; P.n_live = live_irregular(S, min_oligo_length);
	int rc;
	// The second form of the seed scan (pcr_scan_seed2.inc) takes the pass when no 5'/3' shift candidates are asked for and
	// the orientations and their 9-gram seeds fit its LDS budget; the host then only LISTS the seeds (from a cache keyed by
	// oligo and floor: between two optimiser iterations most oligos stay what they were).
	const bool no_shifts = ctx->scan_version == 3 && !optimize_5 && !optimize_3;
	const bool seed2_ok = no_shifts && !ctx->force_seed1 && n_or <= 65535;
	bool want_seed3 = false;
	if(seed2_ok && !ctx->no_seed3 && !ctx->no_irr_index && ctx->s2_dbg == 0){
		// the position index costs 16 bytes per base and milliseconds to build: a set gets it when the first pass that can use it
		// arrives (every candidate seeded) -- a background set screened at 0.72 never does
		bool worth = true;
		if(!S.pix_valid){
			std::vector<uint32_t> os, op; uint32_t om = 0;
			worth = plan_seed2(ctx, L, cand, os, op, om, nullptr) && op.empty() && !os.empty();
		}
		if(worth){
			if((rc = ensure_pos_index(ctx, S)) != PCR_OK) return rc;
			bool irr_ok = P.n_live == 0;
			if(S.pix_usable && !irr_ok && (rc = irr_index_usable(ctx, S, irr_ok)) != PCR_OK) return rc;
			want_seed3 = S.pix_usable && irr_ok; P.s3_with_irr = P.n_live > 0;
		}
	}
	bool use_seed2 = false;
	if(seed2_ok){
		use_seed2 = plan_seed2(ctx, L, cand, or_seed, or_plain, P.irr_off_mask, want_seed3 ? &S : nullptr);
		if(want_seed3 && !(use_seed2 && or_plain.empty() && !or_seed.empty() && plan_seed3_slices(ctx, L, P.s3_with_irr))){
			// the third form will not take the pass (an unseeded candidate, or its lists do not fit): plan within the second form's limits
			or_seed.clear(); or_plain.clear();
			use_seed2 = plan_seed2(ctx, L, cand, or_seed, or_plain, P.irr_off_mask, nullptr);
		}
		// an orientation without a 9-gram structure (low thresholds: k = 4 mismatching slots and more) may still have an 8-gram
		// one: let the first form plan the pass where it can (it hands fewer orientations to the bit-sliced scan); a batch beyond
		// its S1_MAX_OR orientations keeps this form for the seedable orientations, the others go to the bit-sliced scan
		if(use_seed2 && !or_plain.empty() && (n_or <= S1_MAX_OR || or_seed.empty())) use_seed2 = false;
		if(!use_seed2){ or_seed.clear(); or_plain.clear(); P.irr_off_mask = 0; }
	}
	// ... and the third form -- the targets' positions indexed by their 9-grams, the seeds looked up (pcr_scan_seed3.inc) -- where every
	// candidate is seeded (and the irregular words can come in through their index too: want_seed3, decided before the planning)
	const bool use_seed3 = use_seed2 && want_seed3 && or_plain.empty() && !or_seed.empty()
		&& L.s3_prefix.size() == L.s2_seeds.size() + L.s2_group_end.size() && L.s3_spans.size() == L.s2_seeds.size();
	if(use_seed2){ P.form = use_seed3 ? ScanForm::Seed3 : ScanForm::Seed2; P.n_seeds = L.s2_seeds.size(); }
	else if(no_shifts && !ctx->host_seed_tables && n_or <= S1_MAX_OR){      // first form, tables built by k_seed_tables
		plan_seed1(ctx, L, cand, or_seed, or_plain, P.irr_off_mask);
		P.form = ScanForm::Seed1Dev; P.n_seeds = L.s1_seeds.size();
	}
	else if(ctx->scan_version == 3 && n_or <= 65535){
		const int prc = plan_seed_host(ctx, cand, P.H, or_seed, or_plain, P.irr_off_mask);
		// (the counters the table build touched are cleared again whatever happened: they stay all-zero between passes)
		if(ctx->seed_count.size() == 65536){ for(const pcrhost::Seed &sd : P.H.seeds){ ctx->seed_count[sd.code] = 0; ctx->seed_own[sd.code] = 0; } }
		if(prc != PCR_OK) return prc;
		P.form = ScanForm::Seed1Host; P.n_seeds = P.H.seeds.size() + P.H.n_inherited;
	}
	else{
		for(uint32_t o = 0;o < n_or;++o) or_plain.push_back(o);
		P.form = (ctx->scan_version == 1) ? ScanForm::Popcount : ScanForm::BitSliced;
	}
	if(or_seed.empty() && P.form != ScanForm::Popcount) P.form = ScanForm::BitSliced;
	P.need_plain = (ctx->scan_version != 1) && !or_plain.empty();
	P.need_seedset = !or_seed.empty() && S.n_degen_tiles > 0;
	return PCR_OK;
}

// One pass, self-contained: the call's arguments, everything its planning made, and what the device stage needs to run it.
// The caller's thread fills it (plan_pass: stage A), the thread that runs run_pass reads it (stage B): the same thread for an
// inline pass, the stream's launcher thread for a pipelined one.  Recycled through a free list per handle.
//
// WHO OWNS WHAT while a handle has jobs in its stream's launch queue
//   caller thread (stage A): argument checks; build_candidates; the planning half of choose_scan_form with the per-oligo caches
//     (seed_lists: the second and third forms' caches, each with its positional memo, and the listing's scratch; s1_cache, s2_tmp,
//     seed_count/own/fill); plan_seed3_slices; prepare_tables (candidate planes, floors, build_oligos);
//     pending[]; mail_seq (a pipelined pass's sequence number is reserved at enqueue: the passes of a handle are strictly FIFO);
//     the job free list (under job_m).
//   launcher thread (stage B): the Stager rings with their wait_published spin; the sizing of S.ctrl / hits / S.db / best / S.touched;
//     the lean decision and the epoch; every launch; S.ctrl_clean, touched_from_seg, touched_built, d_seg_hi and the have_db markers
//     (have_db, n_entries, n_touched, db_cap, n_slots); d_cand_*; the profiling events; t_host[1], t_host[2].
//   set state that stage A READS (pix_*, pix_start_h, irx_valid, irr_size_count, irr_n_multi, n_irr, n_degen_tiles, n, bucket_cap)
//     is written only while the queue holds no job of the handle: every writer sits behind DRAIN / flush_launcher.
struct PassJob {
	// the call
	pcr_ctx *ctx = nullptr; int which = 0, opt5 = 0, opt3 = 0; float thr = 0.0f; uint32_t min_len = 0; bool async = false;
	pcr_amplify_args args = {}; FusedAmp fa = {}; bool has_fa = false;
	uint32_t seq = 0;                                 // the pass's reserved mailbox sequence number; 0: the tail takes the next one (inline passes)
	bool begun = false, ctrl_was_clean = false;       // inline passes: begin_pass() ran before the planning, as it always has
	// the plan
	std::vector<pcrhost::Candidate> cand; ScanPlan P; PlanLists L;
	std::vector<uint4> hf, hr; std::vector<uint32_t> hfl;   // candidate planes and floors as the device reads them
	std::vector<OligoDev> ol;                         // fused pass: the amplicon screen's oligo table
	bool fuse = false; size_t bits_bytes = 0;         // fuse: the screen rides in the pass; bytes of each of its two result bitsets
	// stage B, when the pass is one half of a paired launch (pair_slices): the slices of its half grid
	Seed3HalfSlices pair_W; uint32_t pair_slice_cap = 0;
	void reset()
	{
		seq = 0; begun = ctrl_was_clean = false; has_fa = false; fa = FusedAmp(); async = false;
		cand.clear(); P.reset(); L.clear(); hf.clear(); hr.clear(); hfl.clear(); ol.clear(); fuse = false; bits_bytes = 0;
	}
};

// What the launches of a pass read on the device (stage_tables).
struct Scan2Staged { Scan2Tables T; const uint32_t *d_tab = nullptr, *d_bias = nullptr, *d_map = nullptr; };
struct StagedTables {
	SeedTables ST = {};
	Seed2Tables ST2 = {};
	const uint32_t *d_s3_prefix = nullptr; const uint8_t *d_s3_spans = nullptr;
	Scan2Staged plain, seedset;
	bool lean = false, fuse = false;                  // lean: the fused pass without a staging launch (see pcr_ctx::dstage)
	size_t bits_bytes = 0;                            // of each of the fused pass's two result bitsets
};

void stage_scan2(Stager &st, const std::vector<uint32_t> &orients, Scan2Staged &B)
{
	B.d_tab = st.put(B.T.tab.data(), B.T.tab.size());
	B.d_bias = st.put(B.T.bias.data(), B.T.bias.size());
	std::vector<uint32_t> m(orients);
	m.resize((m.size() + 255) & ~size_t(255), 0xFFFFFFFFu);
	B.d_map = st.put(m.data(), m.size());
}

// Stage A's last step: the host tables that depend on nothing but the call -- candidate planes and floors in device layout, the
// second form's floor bytes, and for a fused pass the amplicon screen's oligo table.  (S is only asked for its size.)
void prepare_tables(const SeqSet &S, PassJob &J, FusedAmp *fa)
{
	const std::vector<pcrhost::Candidate> &cand = J.cand;
	const uint32_t ncand = (uint32_t)cand.size(), n_or = 2*ncand;
	J.hf.resize(ncand); J.hr.resize(ncand); J.hfl.resize(ncand);
	for(uint32_t c = 0;c < ncand;++c){
		J.hf[c] = make_uint4(cand[c].fwd.a, cand[c].fwd.c, cand[c].fwd.g, cand[c].fwd.t);
		J.hr[c] = make_uint4(cand[c].rc.a, cand[c].rc.c, cand[c].rc.g, cand[c].rc.t);
		J.hfl[c] = cand[c].floor_;
	}
	if(is_seed2(J.P.form)){
		// (the mask entries come out of the per-oligo cache: plan_seed2)
		std::vector<uint8_t> &floors2 = J.L.s2_floors;
		floors2.assign(((size_t)n_or + 15) & ~size_t(15), 0);
		for(uint32_t o = 0;o < n_or;++o) floors2[o] = (uint8_t)std::min<uint32_t>(cand[o >> 1].floor_, 255u);
	}
	// fused pass: the amplicon screen's oligo table travels with the scan tables, its result bitsets are
	// cleared by the same launch
	J.fuse = false; J.bits_bytes = 0; J.ol.clear();
	if(fa && fa->n_pairs){
		J.bits_bytes = (size_t)fa->n_pairs*((S.n + 63)/64)*sizeof(uint64_t);
		J.fuse = ((uintptr_t)fa->d_fr % 16 == 0) && ((uintptr_t)fa->d_rf % 16 == 0) && (J.bits_bytes % 16 == 0);
		if(J.fuse) build_oligos(fa->pairs, fa->n_pairs, fa->a, J.ol);
	}
}

// Stage B's first step: the pass's tables to the device (a ring slot, k_stage or the lean form's direct write).
int stage_tables(pcr_ctx *ctx, SeqSet &S, const PassJob &J, FusedAmp *fa, bool async, bool ctrl_was_clean, StagedTables &T)
{
	const std::vector<pcrhost::Candidate> &cand = J.cand;
	const ScanPlan &P = J.P; const PlanLists &L = J.L;
	const uint32_t ncand = (uint32_t)cand.size(), n_or = 2*ncand;
	const bool seed2 = is_seed2(P.form), seed3 = P.form == ScanForm::Seed3;
	const bool build_tables = P.form == ScanForm::Seed1Dev;
	const HostSeedPlan &H = P.H;
	int rc;
	if(P.need_plain) build_scan2_tables(cand, P.or_plain, T.plain.T);
	if(P.need_seedset) build_scan2_tables(cand, P.or_seed, T.seedset.T);
	size_t bytes = ncand*(2*sizeof(uint4) + sizeof(uint32_t)) + 1024;
	bytes += (T.plain.T.tab.size() + T.plain.T.bias.size() + P.or_plain.size() + 256)*sizeof(uint32_t);
	bytes += (T.seedset.T.tab.size() + T.seedset.T.bias.size() + P.or_seed.size() + 256)*sizeof(uint32_t);
	bytes += (H.image.size() + H.heads.size() + H.multi.size() + 64)*sizeof(uint32_t);
	if(seed2){
		bytes += L.s2_masks.size()*sizeof(uint4) + L.s2_floors.size() + L.s2_seeds.size()*sizeof(uint32_t) + 512;
		if(seed3) bytes += L.s3_prefix.size()*sizeof(uint32_t) + L.s3_spans.size() + 128;
	}
	if(build_tables) bytes += L.s1_seeds.size()*sizeof(uint32_t) + 256;
	T.bits_bytes = J.bits_bytes; T.fuse = J.fuse;
	if(T.fuse) bytes += J.ol.size()*sizeof(OligoDev) + 64;
	const uint32_t guard_seq = J.seq ? J.seq : ctx->mail_seq + 1;   // the sequence number the pass's tail will publish
	// the pass's control block (counters | per-sequence fills | segment ends)
	const uint64_t gen = S.ctrl.generation;
	if((rc = S.ctrl.ensure(8 + 2*(size_t)S.n + 4)) != PCR_OK) return rc;
	T.lean = ctx->direct_ok && async && T.fuse && seed2 && !P.or_seed.empty() && ctrl_was_clean && gen == S.ctrl.generation
		&& S.bucket_cap == POST_CAP && 2*fa->n_pairs <= 32*POST_MASK_WORDS;
	if(ctx->debug_log) fprintf(stderr, "[pcramp] staging: %s\n", T.lean ? "lean (tables written into device memory, no staging launch)" : "k_stage");
	Stager st(ctx);
	if((rc = T.lean ? st.begin_direct(bytes) : st.begin(bytes)) != PCR_OK) return rc;
	ctx->d_cand_fwd = st.put(J.hf.data(), ncand);
	ctx->d_cand_rc = st.put(J.hr.data(), ncand);
	ctx->d_cand_floor = st.put(J.hfl.data(), ncand);
	if(P.need_plain) stage_scan2(st, P.or_plain, T.plain);
	if(P.need_seedset) stage_scan2(st, P.or_seed, T.seedset);
	if(!H.image.empty()){
		T.ST.image = st.put(H.image.data(), H.image.size());
		T.ST.heads = st.put(H.heads.data(), H.heads.size());
		T.ST.multi = H.multi.empty() ? T.ST.heads : st.put(H.multi.data(), H.multi.size());
	}
	const uint32_t *d_s1_seeds = nullptr;
	if(build_tables){
		d_s1_seeds = st.put(L.s1_seeds.data(), L.s1_seeds.size());
		if((rc = ctx->s1_image.ensure(SEED_IMAGE_WORDS)) != PCR_OK) return rc;
		if((rc = ctx->s1_heads.ensure(2*(size_t)S1_MAX_SEEDS)) != PCR_OK) return rc;   // two words per distinct code
		if((rc = ctx->s1_multi.ensure(S1_MAX_SEEDS)) != PCR_OK) return rc;
		T.ST.image = ctx->s1_image.p; T.ST.heads = ctx->s1_heads.p; T.ST.multi = ctx->s1_multi.p; T.ST.flat = 1;
	}
	if(seed2){
		T.ST2.seeds = st.put(L.s2_seeds.data(), L.s2_seeds.size());
		T.ST2.masks = st.put(reinterpret_cast<const uint4 *>(L.s2_masks.data()), L.s2_masks.size());
		T.ST2.floors = st.put(L.s2_floors.data(), L.s2_floors.size());
		T.ST2.n_seeds = (uint32_t)L.s2_seeds.size(); T.ST2.n_or = n_or;
		if(seed3){ T.d_s3_prefix = st.put(L.s3_prefix.data(), L.s3_prefix.size()); T.d_s3_spans = st.put(L.s3_spans.data(), L.s3_spans.size()); }
	}
	// the staging launch also clears the control block and the result bitsets -- unless the pass is lean: then the tables
	// are already in device memory, the control block was left clean by the previous pass's tail and the first scan launch
	// clears the bitsets
	const size_t ctrl_bytes = (8 + 2*(size_t)S.n)*sizeof(uint32_t);
	if(T.fuse){
		fa->d_oligos = st.put(J.ol.data(), J.ol.size());
		fa->staged = true;
		if(T.lean) st.seal(guard_seq);
		else if((rc = st.ship(S.ctrl.p, ctrl_bytes, fa->d_fr, T.bits_bytes, fa->d_rf, T.bits_bytes, guard_seq)) != PCR_OK) return rc;
	}
	else if((rc = st.ship(S.ctrl.p, ctrl_bytes, nullptr, 0, nullptr, 0, guard_seq)) != PCR_OK) return rc;
	if(build_tables){
		if((rc = ctx->s1_part.ensure(2*S1_GROUPS)) != PCR_OK) return rc;
		hipLaunchKernelGGL(k_seed_tables<false>, dim3(S1_GROUPS), dim3(S1_BUILD_THREADS), 0, ctx->stream, d_s1_seeds, (uint32_t)L.s1_seeds.size(),
			ctx->s1_part.p, ctx->s1_image.p, ctx->s1_heads.p, ctx->s1_multi.p);
		hipLaunchKernelGGL(k_seed_tables<true>, dim3(S1_GROUPS), dim3(S1_BUILD_THREADS), 0, ctx->stream, d_s1_seeds, (uint32_t)L.s1_seeds.size(),
			ctx->s1_part.p, ctx->s1_image.p, ctx->s1_heads.p, ctx->s1_multi.p);
		HIP_TRY(hipGetLastError());
	}
	return PCR_OK;
}

// ---- launches: one function per form; each appends its hits to `sink`

int launch_popcount(pcr_ctx *ctx, SeqSet &S, const HitSink &sink)
{
	hipLaunchKernelGGL(k_scan, dim3(S.n_tiles), dim3(SCAN_THREADS), 0, ctx->stream, S.planes.p, S.valid_d(),
		S.d_blk_off.p, S.d_len.p, S.d_active.p, S.tile_seq.p, S.tile_pos0.p, ctx->d_cand_fwd, ctx->d_cand_rc,
		ctx->d_cand_floor, sink.ncand, sink);
	HIP_TRY(hipGetLastError());
	return PCR_OK;
}

// First form (pcr_scan_seed.inc), tables built on the host or by k_seed_tables.
int launch_seed1(pcr_ctx *ctx, SeqSet &S, const ScanPlan &P, const StagedTables &T, const HitSink &sink)
{
	const uint32_t ncand = sink.ncand;
	const bool cand_lds = ncand <= SEED_CAND_LDS;   // (candidates read from global to fit 8 workgroups per CU: 140 vs 102 us)
	const auto kernel = cand_lds ? k_seed<true> : k_seed<false>;
	const size_t dyn = cand_lds ? (size_t)ncand*(2*sizeof(uint4) + sizeof(uint32_t)) : 0;
	// persistent workgroups: exactly as many as are resident at once (a partial second round would
	// run alone at the end), asked of the runtime for this kernel and its dynamic LDS size
	int per_cu = 0;
	const hipError_t oe = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, SEED_THREADS, dyn);
	// The runtime's answer was one too high twice (7 for 21.6 KB of LDS, 6 for 27.2 KB: the extra workgroup
	// ran as a second round, 146 vs 109 us at C2); both cases fit "160 KB, allocated in 4 KB units".
	const size_t lds_wg = ((sizeof(SeedShared) + dyn + 4095)/4096)*4096;
	per_cu = std::max(1, std::min<int>(per_cu, (int)((160*1024)/lds_wg)));
	const uint32_t resident = (oe == hipSuccess) ? (uint32_t)per_cu*ctx->n_cu : SEED_MAX_GRID;
	const uint32_t tiles_per_wg = SEED_WAVES*SEED_TILES_PER_WAVE;
	const dim3 sgrid(std::min<uint32_t>((S.n_tiles + tiles_per_wg - 1)/tiles_per_wg, resident)), sblock(SEED_THREADS);
	// the irregular words ride along as extra workgroups behind the persistent ones: they fill the
	// issue slots the latency-bound seed scan leaves idle instead of running alone afterwards
	IrrArgs IA; IA.irr = S.irr.p; IA.perm = S.irr_perm.p; IA.n_live = P.n_live; IA.off_mask = P.or_plain.empty() ? P.irr_off_mask : 0u;   // the seeded irregular scan needs every candidate seeded
	const uint32_t irr_wgs = (P.n_live + IRR_THREADS*IRR_PER_LANE - 1)/(IRR_THREADS*IRR_PER_LANE);
	const dim3 fgrid(sgrid.x + irr_wgs);
	if(ctx->debug_log) fprintf(stderr, "[pcramp] k_seed: %d workgroups per CU x %u CUs\n", per_cu, ctx->n_cu);
	hipLaunchKernelGGL(kernel, fgrid, sblock, dyn, ctx->stream, S.tb_d(), S.planes.p, S.valid_d(), S.d_blk_off.p, S.d_nblk_real.p, S.d_len.p, S.d_active.p,
		S.tile_seq.p, S.tile_pos0.p, S.tile_degen.p, S.n_tiles, T.ST, ctx->d_cand_fwd, ctx->d_cand_rc, ctx->d_cand_floor, ncand, IA, sgrid.x, sink);
	HIP_TRY(hipGetLastError());
	return PCR_OK;
}

// Third form: what the launch of one seed group reads (its slices: plan_seed3_slices), and the dynamic LDS it asks for.
void seed3_args(SeqSet &S, const Seed2Tables &Tg, const uint32_t *d_chunk_prefix, const uint8_t *d_spans, const pcr_ctx::S3Launch &L3, const IrrArgs2 &IA, Seed3Tables &T3, Seed3Set &Q3)
{
	T3.seeds = Tg.seeds; T3.spans = d_spans; T3.chunk_prefix = d_chunk_prefix; T3.masks = Tg.masks; T3.floors = Tg.floors;
	T3.n_seeds = Tg.n_seeds; T3.n_or = Tg.n_or; T3.or_base = Tg.or_base;
	T3.pix_first = S.pix_first.p; T3.pix_last = S.pix_last.p; T3.pix_ent = S.pix_ent.p;
	Q3 = Seed3Set{ S.valid_d(), S.blk_info.p, S.blk_local.p, S.d_active.p };
	T3.n_chunks = L3.n_chunks; T3.per_wg = L3.per_wg; T3.slice_cap = L3.slice_cap;
	T3.n_irr_wg = IA.ix_first ? L3.n_irr_wg : 0u;           // (without the index the chunk workgroups are fewer than they could be: harmless)
}
inline size_t seed3_lds(const Seed3Tables &T3)
{
	return (size_t)T3.n_or*sizeof(uint4) + 2*(size_t)T3.slice_cap*sizeof(uint32_t) + (((size_t)T3.n_or + 15) & ~size_t(15)) + (((size_t)T3.slice_cap + 15) & ~size_t(15)) + 16;
}

// Third form: the launch of one seed group.
int launch_seed3_group(pcr_ctx *ctx, SeqSet &S, const Seed2Tables &Tg, const uint32_t *d_chunk_prefix, const uint8_t *d_spans, const pcr_ctx::S3Launch &L3, const IrrArgs2 &IA,
	const HitSink &sink, const S2Clear &Z)
{
	Seed3Tables T3; Seed3Set Q3;
	seed3_args(S, Tg, d_chunk_prefix, d_spans, L3, IA, T3, Q3);
	const size_t dyn3 = seed3_lds(T3);
	if(!ctx->s3_attr_set){
		HIP_TRY(hipFuncSetAttribute((const void *)k_seed3<S3_WG_THREADS>, hipFuncAttributeMaxDynamicSharedMemorySize, 128*1024));
		ctx->s3_attr_set = true;
	}
	hipLaunchKernelGGL(k_seed3<S3_WG_THREADS>, dim3(seed3_grid(ctx)), dim3(S3_WG_THREADS), dyn3, ctx->stream, T3, Q3, IA, ctx->d_cand_fwd, ctx->d_cand_floor, sink, Z, L3.W);
	return PCR_OK;
}

// How the irregular words of the set reach the launch of one seed group of the second or third form.
IrrArgs2 group_irr_args(SeqSet &S, const ScanPlan &P, uint32_t group_offmask, bool first_launch, bool irr_by_index)
{
	IrrArgs2 IA; IA.scan = S.irr_scan.p; IA.irr = S.irr.p; IA.n_live = P.n_live;
	IA.off_mask = group_offmask;
	IA.exhaustive = first_launch ? 1u : 0u;                             // words holding IUPAC slots meet every candidate once, in the first launch
	IA.ix_first = IA.ix_last = IA.ix_words = nullptr; IA.min_cws = std::min<uint32_t>(P.min_len, 255u);
	if(!P.or_plain.empty()){                                            // unseeded candidates in the pass: every irregular word meets every candidate, once
		IA.off_mask = 0;
		if(!first_launch) IA.n_live = 0;
	}
	else if(irr_by_index){                                               // every candidate seeded, no IUPAC word in the set: the words come in through the index, by seed
		IA.ix_first = S.irx_first.p; IA.ix_last = S.irx_last.p; IA.ix_words = S.irx_words.p; IA.n_live = 0;
	}
	return IA;
}
// What the launch clears in its prologue: the first launch of a lean pass clears the result bitsets.
S2Clear group_clear(const StagedTables &T, const FusedAmp *fa, const HitSink &sink, bool first_launch)
{
	S2Clear Z = { nullptr, 0u, nullptr, 0u, nullptr };
	if(T.lean && first_launch){
		Z.z0 = (uint4 *)fa->d_fr; Z.z1 = (uint4 *)fa->d_rf; Z.n0 = Z.n1 = (uint32_t)(T.bits_bytes/16); Z.ctrl = sink.counters;
	}
	return Z;
}

// Second and third form: one launch per seed group (plan_seed2).  The second form runs persistent workgroups of 16 waves, one per
// CU (the tables they build take most of its LDS); the irregular words are taken by the same waves once their tiles are done.
int launch_seed_groups(pcr_ctx *ctx, SeqSet &S, const ScanPlan &P, const PlanLists &L, const StagedTables &T, const FusedAmp *fa, const HitSink &sink)
{
	const bool seed3 = P.form == ScanForm::Seed3;
	const uint32_t tiles_per_wg = S2_WAVES*2;
	const dim3 sgrid(std::max<uint32_t>(1u, std::min<uint32_t>((S.n_tiles + tiles_per_wg - 1)/tiles_per_wg, ctx->n_cu))), sblock(S2_THREADS);
	int rc;
	if(!ctx->s2_attr_set){
		HIP_TRY(hipFuncSetAttribute((const void *)k_seed2<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(160*1024 - sizeof(S2Shared))));
		HIP_TRY(hipFuncSetAttribute((const void *)k_seed2<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(160*1024 - sizeof(S2Shared))));
		ctx->s2_attr_set = true;
	}
	const auto k_seed2_of_ctx = ctx->s2_dbg ? k_seed2<true> : k_seed2<false>;   // (<true>: the ablation build, PCRAMP_S2DBG)
	bool irr_by_index = P.s3_with_irr;                    // third form: decided with the form, the index is there and usable
	if(!seed3){
		irr_by_index = P.or_plain.empty() && P.n_live > 0 && !ctx->no_irr_index;
		for(size_t g = 0, b = 0;g < L.s2_group_end.size();++g){ if((size_t)L.s2_group_end[g] - b > (size_t)sgrid.x*S2_THREADS) irr_by_index = false; b = L.s2_group_end[g]; }   // (a thread looks up at most one seed)
		if(irr_by_index && (rc = irr_index_usable(ctx, S, irr_by_index)) != PCR_OK) return rc;
	}
	uint32_t g_begin = 0, g_prefix = 0;
	bool first_launch = true;
	for(size_t g = 0;g < L.s2_group_end.size();++g){
		Seed2Tables Tg = T.ST2;
		const uint32_t or0 = L.s2_group_or[g], g_or = L.s2_group_nor[g];
		const uint8_t *const d_spans = seed3 ? T.d_s3_spans + g_begin : nullptr;         // (the group's offset in the seed list is the spans' too)
		Tg.seeds = T.ST2.seeds + g_begin; Tg.n_seeds = L.s2_group_end[g] - g_begin;
		Tg.masks = T.ST2.masks + (size_t)or0; Tg.floors = T.ST2.floors + or0; Tg.n_or = g_or; Tg.or_base = or0;
		g_begin = L.s2_group_end[g];
		if(Tg.n_seeds == 0){ g_prefix += 1u; continue; }
		const size_t dyn = (size_t)g_or*sizeof(uint4) + (((size_t)g_or + 15) & ~size_t(15)) + 8*((size_t)Tg.n_seeds + 64) + 16;   // masks | floors | chain | head (each with 64 dummy slots)
		const IrrArgs2 IA = group_irr_args(S, P, L.s2_group_offmask[g], first_launch, irr_by_index);
		if(ctx->debug_log) fprintf(stderr, "[pcramp] k_seed2: %u workgroups, %u seeds of orientations %u..%u (group %zu of %zu), %zu + %zu B of LDS\n", sgrid.x, Tg.n_seeds,
			or0, or0 + g_or - 1, g + 1, L.s2_group_end.size(), sizeof(S2Shared), dyn);
		const S2Clear Z = group_clear(T, fa, sink, first_launch);
		if(seed3){
			if((rc = launch_seed3_group(ctx, S, Tg, T.d_s3_prefix + g_prefix, d_spans, L.s3_launch[g], IA, sink, Z)) != PCR_OK) return rc;
			g_prefix += Tg.n_seeds + 1u;
		}
		else hipLaunchKernelGGL(k_seed2_of_ctx, sgrid, sblock, dyn, ctx->stream, S.tb_d(), S.valid_d(), S.tile_desc.p, S.n_tiles, Tg, S.d_active.p, ctx->d_cand_fwd, ctx->d_cand_floor,
			sink.ncand, IA, sink, ctx->s2_dbg, Z);
		HIP_TRY(hipGetLastError());
		first_launch = false;
	}
	return PCR_OK;
}

// The irregular words on their own: the forms that have no seed scan to carry them along.
int launch_irregular(pcr_ctx *ctx, SeqSet &S, const ScanPlan &P, const HitSink &sink)
{
	const unsigned irr_grid = (P.n_live + IRR_THREADS*IRR_PER_LANE - 1)/(IRR_THREADS*IRR_PER_LANE);
	hipLaunchKernelGGL(k_scan_irr, dim3(irr_grid), dim3(IRR_THREADS), 0, ctx->stream, S.irr.p, S.irr_perm.p, P.n_live,
		S.d_active.p, ctx->d_cand_fwd, ctx->d_cand_floor, sink.ncand, sink);
	HIP_TRY(hipGetLastError());
	return PCR_OK;
}

// All scan launches of one attempt: bit-sliced counter for the unseeded orientations, the plan's form for the seeded ones, the
// bit-sliced counter again for those in the IUPAC tiles, then the irregular words where no seed scan took them along.
int launch_scans(pcr_ctx *ctx, SeqSet &S, const ScanPlan &P, const PlanLists &L, const StagedTables &T, const FusedAmp *fa, const HitSink &sink)
{
	int rc = PCR_OK;
	const uint32_t ncand = sink.ncand;
	if(S.n_tiles){
		// events around the scan launches of every prof_stride-th pass (an event between two kernels costs a ~6 us queue bubble)
		ProfScope scan_prof(ctx, PCR_PROF_SCAN, ctx->prof && (ctx->prof_pass++ % ctx->prof_stride) == 0);
		if(P.need_plain && (rc = launch_scan2(ctx, S, T.plain.T, ncand, sink, T.plain.d_tab, T.plain.d_bias, nullptr, S.n_tiles, T.plain.d_map)) != PCR_OK) return rc;
		if(P.form == ScanForm::Popcount) rc = launch_popcount(ctx, S, sink);
		else if(is_seed1(P.form)) rc = launch_seed1(ctx, S, P, T, sink);
		else if(is_seed2(P.form)) rc = launch_seed_groups(ctx, S, P, L, T, fa, sink);
		if(rc != PCR_OK) return rc;
		if(P.need_seedset && (rc = launch_scan2(ctx, S, T.seedset.T, ncand, sink, T.seedset.d_tab, T.seedset.d_bias, S.degen_tiles.p, S.n_degen_tiles,
			T.seedset.d_map)) != PCR_OK) return rc;
		scan_prof.finish();
	}
	const bool irr_taken = S.n_tiles && (is_seed1(P.form) || is_seed2(P.form));   // by extra workgroups of k_seed / by the waves of k_seed2, k_seed3
	if(P.n_live && !irr_taken) rc = launch_irregular(ctx, S, P, sink);
	return rc;
}

// ---- tails

// The whole tail -- DB finalisation and the amplicon screen -- in one launch: k_post (64-slot buckets, WAVES sequences per
// workgroup) or k_post_big (128 / 256 slots).
PostRow post_row_args(pcr_ctx *ctx, SeqSet &S, const HitSink &sink, const FusedAmp *fa, uint32_t seq)
{
	PostRow R;
	R.hits = sink.hits; R.seq_count = sink.seq_count; R.best = sink.best; R.ncand = sink.ncand; R.planes = S.planes.p; R.blk_off = S.d_blk_off.p;
	R.irr = S.irr.p; R.irr_off = S.irr_off.p; R.db = S.db.p; R.seg_hi = S.d_seg_hi; R.counters = sink.counters; R.epoch = sink.epoch; R.n_seq = S.n;
	R.oligos = fa->d_oligos; R.n_pairs = fa->n_pairs; R.mask_words = (2*fa->n_pairs + 31)/32; R.len = S.d_len.p; R.active = S.d_active.p;
	R.amp_min = fa->a->amp_min; R.amp_max = fa->a->amp_max; R.ident_thr = fa->a->ident_threshold; R.use_taq = fa->a->use_taq_mama;
	R.bits_fr = fa->d_fr; R.bits_rf = fa->d_rf; R.bit_words = (uint64_t)((S.n + 63)/64); R.pub_mail = ctx->mail.dev + (seq % pcr_ctx::MAIL_RING); R.pub_seq = seq;
	return R;
}
template<class K>
void launch_post(K kernel, uint32_t waves, pcr_ctx *ctx, SeqSet &S, const HitSink &sink, const FusedAmp *fa, uint32_t seq)
{
	const PostRow R = post_row_args(ctx, S, sink, fa, seq);
	hipLaunchKernelGGL(kernel, dim3((S.n + waves - 1)/waves), dim3(64*waves), 0, ctx->stream, R.hits, R.seq_count, R.best, R.ncand, R.planes,
		R.blk_off, R.irr, R.irr_off, R.db, R.seg_hi, R.counters, R.epoch, R.n_seq,
		R.oligos, R.n_pairs, R.mask_words, R.len, R.active, R.amp_min, R.amp_max,
		R.ident_thr, R.use_taq, R.bits_fr, R.bits_rf, R.bit_words, R.pub_mail, R.pub_seq);
}
// reserved_seq: the sequence number a pipelined pass was given at enqueue; 0: the next one
int fused_tail(pcr_ctx *ctx, SeqSet &S, const HitSink &sink, FusedAmp *fa, uint32_t reserved_seq)
{
	const uint32_t seq = reserved_seq ? reserved_seq : ++ctx->mail_seq;
	if(sink.cap == POST_CAP){
		// 8 waves per workgroup: 4 and 16 measured within the noise of 8 (profiles/dbg/r03_ab_post_waves.txt)
		launch_post(k_post<8>, 8, ctx, S, sink, fa, seq);
		S.ctrl_clean = true; S.touched_from_seg = true;              // k_post zeroes the counters and fills it has read
	}
	else if(sink.cap == 128) launch_post(k_post_big<128, 4>, 4, ctx, S, sink, fa, seq);
	else launch_post(k_post_big<256, 4>, 4, ctx, S, sink, fa, seq);
	HIP_TRY(hipGetLastError());
	fa->posted = true;
	S.touched_built = false;
	return PCR_OK;
}

template<class K, class... Extra>
void launch_finalize(K kernel, dim3 grid, dim3 block, size_t lds, pcr_ctx *ctx, SeqSet &S, const HitSink &sink, Extra... extra)
{
	hipLaunchKernelGGL(kernel, grid, block, lds, ctx->stream, sink.hits, sink.seq_count, sink.cap, sink.best, sink.ncand, S.planes.p, S.d_blk_off.p, S.irr.p,
		S.irr_off.p, S.db.p, S.d_seg_hi, sink.counters, sink.epoch, S.touched.p, extra...);
}
// k_touched, the k_finalize the bucket size asks for, then the counters to the host's mailbox: by k_publish, or -- fused pass --
// by the k_match that follows.  ALL: the all-sites pass (pcr_select_sites.inc), whose finalize keeps every hit.
template<bool ALL = false>
int plain_tail(pcr_ctx *ctx, SeqSet &S, const HitSink &sink, bool async, FusedAmp *fa)
{
	int rc;
	hipLaunchKernelGGL(k_touched, dim3((S.n + 255)/256), dim3(256), 0, ctx->stream, sink.seq_count, S.n, sink.counters, S.touched.p);
	HIP_TRY(hipGetLastError());
	S.touched_built = true;
	uint32_t np2 = 1; while(np2 < sink.cap) np2 <<= 1;
	if(np2 <= 1024) launch_finalize(k_finalize<FIN_WAVES, ALL>, dim3((S.n + FIN_WAVES - 1)/FIN_WAVES), dim3(64*FIN_WAVES), (size_t)FIN_WAVES*np2*sizeof(uint64_t), ctx, S, sink);
	else if(np2 <= MAX_BUCKET_CAP) launch_finalize(k_finalize<1, ALL>, dim3(S.n), dim3(64), (size_t)np2*sizeof(uint64_t), ctx, S, sink);
	else{
		if((rc = ctx->fin_scratch.ensure((size_t)S.n*np2)) != PCR_OK) return rc;
		launch_finalize(k_finalize_big<ALL>, dim3(S.n), dim3(FINBIG_THREADS), 0, ctx, S, sink, ctx->fin_scratch.p);
	}
	HIP_TRY(hipGetLastError());
	// the only host synchronisation of the pass: overflow flag + DB size, through the mapped mailbox
	++ctx->mail_seq;
	if(async && fa && fa->staged){ fa->pub_seq = ctx->mail_seq; fa->pub_counters = sink.counters; }   // k_match publishes
	else{
		hipLaunchKernelGGL(k_publish, dim3(1), dim3(64), 0, ctx->stream, sink.counters, ctx->mail.dev + (ctx->mail_seq % pcr_ctx::MAIL_RING), ctx->mail_seq);
		HIP_TRY(hipGetLastError());
	}
	return PCR_OK;
}

// The buckets the next attempt should have, or 0: the pass stands.  `overflowed`: some sequence collected more hits than its
// bucket holds.  Otherwise: buckets grown for an earlier, denser pass over this set (a DB selected with every slot shift, a lower
// threshold) make every consumer of this DB walk mostly empty slots (the local search: 3x slower on 2 048-slot buckets holding
// <= 200 entries; their slot-per-thread kernels start a thread per slot): when a quarter of them would do, the pass is repeated
// once with those.
uint32_t resized_buckets(bool overflowed, uint32_t cap, uint32_t largest_fill, int attempt)
{
	if(overflowed){
		uint32_t want = cap*2;
		while(want < largest_fill && want < MAX_BUCKET_CAP_GLOBAL) want *= 2;
		return want;
	}
	if(cap <= 64 || attempt >= 12) return 0;
	uint32_t want = 64;
	while(want < largest_fill + largest_fill/16) want *= 2;
	return (want*4 <= cap) ? want : 0;
}

// The buckets a fused tail handles, and the pair count its masks hold.
inline bool fused_tail_fits(uint32_t cap, uint32_t n_pairs) { return (cap == POST_CAP || cap == 128 || cap == 256) && 2*n_pairs <= 32*POST_MASK_WORDS; }
inline bool buckets_fit(uint64_t n_slots) { return n_slots < (uint64_t(1) << 32) && n_slots*(sizeof(Hit) + sizeof(DevEntry)) <= (uint64_t(96) << 30); }

// The markers a pass resets before anything else; returns whether the previous pass's fused tail left the control block clean.
inline bool begin_pass(SeqSet &S)
{
	S.have_db = false; S.n_entries = 0;
	const bool ctrl_was_clean = S.ctrl_clean;
	S.ctrl_clean = false; S.touched_from_seg = false;
	return ctrl_was_clean;
}

// Stage A: candidates, scan plan and host tables of the pass into J -- no launch; device work only where the plan has to build an
// index of the set first (never in a pipelined pass: plans_without_device_work).
int plan_pass(pcr_ctx *ctx, PassJob &J, const pcr_pair *pairs, uint32_t n_pairs)
{
	SeqSet &S = ctx->sets[J.which];
	HostTimer timer(ctx, 0);
	if(ctx->timing) ++ctx->n_timed;
	pcrhost::build_candidates((const uint64_t *)pairs, n_pairs, J.opt5 != 0, J.opt3 != 0, J.thr, J.cand);
	const uint32_t ncand = (uint32_t)J.cand.size();
	if(S.n == 0 || ncand == 0) return PCR_OK;
	int rc;
	if((rc = choose_scan_form(ctx, S, J.cand, J.opt5, J.opt3, J.min_len, J.P, J.L)) != PCR_OK) return rc;
	if(ctx->debug_log) fprintf(stderr, "[pcramp] scan plan: form=%s, %u candidates, %zu seeded orientations (%zu seeds), %zu plain, %u/%u IUPAC tiles, %u-slot buckets\n",
		form_name(J.P.form), ncand, J.P.or_seed.size(), J.P.n_seeds, J.P.or_plain.size(), S.n_degen_tiles, S.n_tiles, S.bucket_cap);
	prepare_tables(S, J, J.has_fa ? &J.fa : nullptr);
	return PCR_OK;
}

// Would planning a default pass over S leave the device alone?  The position index is built (or will not be asked for) and so is
// the index of the irregular words, where a scan may want it.
bool plans_without_device_work(const pcr_ctx *ctx, const SeqSet &S, int opt5, int opt3, uint32_t min_len)
{
	if(ctx->scan_version != 3 || opt5 || opt3 || ctx->force_seed1) return false;             // (not the second or third form anyway)
	const bool may_want_seed3 = !ctx->no_seed3 && !ctx->no_irr_index && ctx->s2_dbg == 0;
	if(may_want_seed3 && !S.pix_valid) return false;
	if(live_irregular(S, min_len) == 0 || ctx->no_irr_index) return true;
	return S.irr_n_multi != 0 || (uint64_t)24*S.n_irr >= (uint64_t(1) << 32) || S.irx_valid;   // irr_index_usable() would build nothing
}

// Can stage B of the planned pass J run on the launcher thread?  A non-empty, fused, asynchronous pass of the second or third
// form whose buckets fit: run_pass then takes exactly one attempt, ends in fused_tail and touches no state stage A reads.
bool pass_is_pipelinable(const pcr_ctx *ctx, const PassJob &J)
{
	const SeqSet &S = ctx->sets[J.which];
	return J.async && J.has_fa && J.fuse && S.n != 0 && !J.cand.empty() && is_seed2(J.P.form)
		&& fused_tail_fits(S.bucket_cap, J.fa.n_pairs) && buckets_fit((uint64_t)S.n*S.bucket_cap);
}

// Stage B in steps, so that two passes of different handles can share their launches (run_pass_pair): stage_pass and size_attempt
// prepare a pass (buffers ensured, ring slot written, epoch taken), pass_enqueued does its bookkeeping once it is on the stream.

// The pass's arg-max table and its tables on the device.  (Non-empty passes only.)
int stage_pass(pcr_ctx *ctx, PassJob &J, bool ctrl_was_clean, StagedTables &T)
{
	SeqSet &S = ctx->sets[J.which];
	int rc;
	if((rc = ctx->best.ensure((size_t)S.n*J.cand.size())) != PCR_OK) return rc;
	if(ctx->best.generation != ctx->best_seen){
		// fresh (uninitialised) storage: clear once; afterwards the epoch tag makes clearing unnecessary
		HIP_TRY(hipMemsetAsync(ctx->best.p, 0, ctx->best.cap*sizeof(uint32_t), ctx->stream));
		ctx->best_seen = ctx->best.generation; ctx->epoch = std::min(ctx->debug_epoch, EPOCH_LIMIT);
	}
	if((rc = stage_tables(ctx, S, J, J.has_fa ? &J.fa : nullptr, J.async, ctrl_was_clean, T)) != PCR_OK) return rc;
	if((rc = S.touched.ensure(S.n)) != PCR_OK) return rc;
	S.d_seg_hi = S.ctrl.p + 8 + S.n;
	return PCR_OK;
}

// The buckets of one attempt at the set's current bucket size, the attempt's epoch, and the sink its launches append to.
int size_attempt(pcr_ctx *ctx, SeqSet &S, const PassJob &J, int attempt, HitSink &sink)
{
	int rc;
	const uint32_t cap = S.bucket_cap;
	const uint64_t n_slots = (uint64_t)S.n*cap;
	if(!buckets_fit(n_slots)){
		assert(J.seq == 0);                              // (pass_is_pipelinable)
		S.bucket_cap = 64;   // (the size that was refused must not stay: the next pass over this set, with other candidates, starts small and grows again)
		g_err = "pcr_select_words: the per-sequence hit buckets would not fit (too many tied sites per sequence)"; return PCR_ERR_CAPACITY;
	}
	if((rc = ctx->hits.ensure(n_slots)) != PCR_OK) return rc;
	if((rc = S.db.ensure(n_slots)) != PCR_OK) return rc;
	if(attempt > 0) HIP_TRY(hipMemsetAsync(S.ctrl.p, 0, (8 + 2*(size_t)S.n)*sizeof(uint32_t), ctx->stream));
	if(ctx->epoch >= EPOCH_LIMIT){
		// the tag (epoch << 8 | count) is about to leave its 24 bits: every stale entry would compare HIGHER than the new
		// pass's hits and swallow them.  Checked per attempt (every bucket-growth retry takes an epoch of its own).
		HIP_TRY(hipMemsetAsync(ctx->best.p, 0, ctx->best.cap*sizeof(uint32_t), ctx->stream));
		ctx->epoch = 0;
	}
	++ctx->epoch;
	sink.best = ctx->best.p; sink.hits = ctx->hits.p; sink.seq_count = S.ctrl.p + 8;
	sink.counters = S.ctrl.p; sink.cap = cap; sink.ncand = (uint32_t)J.cand.size(); sink.epoch = ctx->epoch;
	return PCR_OK;
}

// An asynchronous pass is on the stream: nobody looks at its counters here (the caller has recorded it as pending).
inline void pass_enqueued(SeqSet &S, uint32_t cap)
{
	S.db_cap = cap; S.n_slots = (uint64_t)S.n*cap;
	S.n_touched = N_TOUCHED_UNKNOWN; S.n_entries = 1; S.have_db = true;
}

// Stage B: size the device buffers, stage the tables, launch the scans and the tail.  async: one attempt, nobody looks at the
// counters (pcr_screen_device; the caller has recorded or will record the pass as pending).
int run_pass(pcr_ctx *ctx, PassJob &J, uint64_t *n_entries_out)
{
	SeqSet &S = ctx->sets[J.which];
	FusedAmp *const fa = J.has_fa ? &J.fa : nullptr;
	const bool async = J.async;
	const bool ctrl_was_clean = J.begun ? J.ctrl_was_clean : begin_pass(S);
	const ScanPlan &P = J.P;
	const uint32_t ncand = (uint32_t)J.cand.size();
	if(S.n == 0 || ncand == 0){ S.have_db = true; S.n_touched = 0; return PCR_OK; }
	HostTimer timer(ctx, 1);
	int rc;
	StagedTables T;
	if((rc = stage_pass(ctx, J, ctrl_was_clean, T)) != PCR_OK) return rc;

	timer.next(2);
	uint32_t h_counters[4];
	for(int attempt = 0;;++attempt){
		const uint32_t cap = S.bucket_cap;
		const uint64_t n_slots = (uint64_t)S.n*cap;
		HitSink sink;
		if((rc = size_attempt(ctx, S, J, attempt, sink)) != PCR_OK) return rc;
		const bool fused = async && fa && fa->staged && fused_tail_fits(cap, fa->n_pairs);
		if(J.seq && !fused){ g_err = "pcr_screen_device: a pipelined pass lost its fused tail"; return PCR_ERR_STATE; }   // (pass_is_pipelinable: cannot happen)
		if((rc = launch_scans(ctx, S, P, J.L, T, fa, sink)) != PCR_OK) return rc;
		if((rc = fused ? fused_tail(ctx, S, sink, fa, J.seq) : plain_tail(ctx, S, sink, async, fa)) != PCR_OK) return rc;
		if(async){ pass_enqueued(S, cap); return PCR_OK; }
		timer.next(3);
		if((rc = mail_wait(ctx, ctx->mail_seq, h_counters)) != PCR_OK) return rc;
		timer.next(2);
		S.db_cap = cap; S.n_slots = n_slots;
		const bool overflowed = (h_counters[0] & 1u) != 0;
		if(overflowed && (attempt >= 12 || cap >= MAX_BUCKET_CAP_GLOBAL)){ g_err = "pcr_select_words: more than 65536 candidate sites in one sequence (per-sequence bucket limit)"; return PCR_ERR_CAPACITY; }
		const uint32_t want = resized_buckets(overflowed, cap, h_counters[2], attempt);
		if(!want) break;
		S.bucket_cap = want;   // grow (or shrink) the buckets and redo the pass
	}
	if(ctx->debug_log) fprintf(stderr, "[pcramp] pass done: %u-slot buckets, largest fill %u, %u sequences with entries\n", S.db_cap, h_counters[2], h_counters[3]);
	S.n_touched = h_counters[3];
	S.n_entries = S.n_touched ? 1 : 0;   // "non-empty" marker; the exact count is taken on demand (count_entries)
	S.have_db = true;
	if(n_entries_out){
		if((rc = count_entries(ctx, S)) != PCR_OK) return rc;
		*n_entries_out = S.n_entries;
	}
	return PCR_OK;
}

// ---- two queued passes of different handles as ONE scan launch and ONE tail launch (k_seed3_pair, k_post_pair)
//
// Both kernels of a pass are bound by the latency of a chain of dependent loads, and a stream runs its kernels one after the other:
// while one pass walks its chain the next one waits.  Two passes that share no state walk side by side instead, each on half the
// scan's workgroups.  What a pass records -- hits, fills, DB, bits, mailbox -- is what it records alone.

// Could the planned pass be one half of a pair?  Third form with one launch group and no other scan launch, 64-slot buckets with
// the fused tail, its scan not bracketed by profiling events (a bracketed scan is timed as one pass's: it launches alone).
bool pass_is_pairable(const pcr_ctx *ctx, const PassJob &J)
{
	const SeqSet &S = ctx->sets[J.which];
	return ctx->pair_mode != 0 && pass_is_pipelinable(ctx, J) && J.P.form == ScanForm::Seed3 && J.L.s2_group_end.size() == 1 && J.L.s2_group_end[0] != 0
		&& !J.P.need_plain && !J.P.need_seedset && S.n_tiles != 0 && S.bucket_cap == POST_CAP
		&& !(ctx->prof && ctx->prof_pass % ctx->prof_stride == 0);
}

// The slices of a pass on half the chunk workgroups with twice the share each: workgroup w takes the shares of 2w and 2w + 1 of the
// plan (which has an even number of them), so its slice starts where 2w's does.  false: the widest slice does not fit the LDS.
bool pair_slices(const pcr_ctx *ctx, PassJob &J)
{
	const pcr_ctx::S3Launch &L3 = J.L.s3_launch[0];
	const uint32_t ns = J.L.s2_group_end[0], G = (seed3_grid(ctx) - L3.n_irr_wg) & ~1u, Gh = G/2;
	uint32_t *const st = J.pair_W.start;
	for(uint32_t w = 0;w <= Gh;++w) st[w] = L3.W.start[2*w];
	for(uint32_t w = Gh + 1;w <= S3_MAX_WG/2;++w) st[w] = st[Gh];
	uint32_t cap = 2;
	for(uint32_t w = 0;w < Gh;++w) cap = std::max(cap, std::min(st[w + 1] + 2u, ns + 1u) - st[w]);
	J.pair_slice_cap = cap;
	return 17*(size_t)J.L.s2_group_nor[0] + 9*(size_t)cap + 64 <= S3_LDS_BUDGET;
}

// May A and B (pushed in this order) share their launches?  Different handles -- passes of one handle share its hits and arg-max
// tables --, both pairable, and neither writes where the other does.
bool passes_can_pair(PassJob &A, PassJob &B)
{
	if(A.ctx == B.ctx || !pass_is_pairable(A.ctx, A) || !pass_is_pairable(B.ctx, B)) return false;
	const uintptr_t a[2] = { (uintptr_t)A.fa.d_fr, (uintptr_t)A.fa.d_rf }, b[2] = { (uintptr_t)B.fa.d_fr, (uintptr_t)B.fa.d_rf };
	for(int i = 0;i < 2;++i) for(int j = 0;j < 2;++j){ if(a[i] < b[j] + B.bits_bytes && b[j] < a[i] + A.bits_bytes) return false; }
	return pair_slices(A.ctx, A) && pair_slices(B.ctx, B);
}

// One half of a pair, prepared: everything run_pass does before its launches.
struct PairHalf { pcr_ctx *ctx; PassJob *J; SeqSet *S; StagedTables T; HitSink sink; Seed3Row scan; PostRow post; };
int prepare_half(PairHalf &H)
{
	pcr_ctx *const ctx = H.ctx; PassJob &J = *H.J; SeqSet &S = *H.S;
	const bool ctrl_was_clean = begin_pass(S);
	int rc;
	HostTimer timer(ctx, 1);
	if((rc = stage_pass(ctx, J, ctrl_was_clean, H.T)) != PCR_OK) return rc;
	timer.next(2);
	if((rc = size_attempt(ctx, S, J, 0, H.sink)) != PCR_OK) return rc;
	if(!J.fa.staged || H.sink.cap != POST_CAP){ g_err = "pcr_screen_device: a paired pass lost its fused tail"; return PCR_ERR_STATE; }   // (pass_is_pairable: cannot happen)
	if(ctx->prof) ++ctx->prof_pass;                       // (not bracketed: pass_is_pairable)
	// the launch's only seed group, as launch_seed_groups makes it
	const PlanLists &L = J.L;
	Seed2Tables Tg = H.T.ST2;
	Tg.n_seeds = L.s2_group_end[0]; Tg.masks = H.T.ST2.masks + (size_t)L.s2_group_or[0]; Tg.floors = H.T.ST2.floors + L.s2_group_or[0];
	Tg.n_or = L.s2_group_nor[0]; Tg.or_base = L.s2_group_or[0];
	H.scan.IA = group_irr_args(S, J.P, L.s2_group_offmask[0], true, J.P.s3_with_irr);
	seed3_args(S, Tg, H.T.d_s3_prefix, H.T.d_s3_spans, L.s3_launch[0], H.scan.IA, H.scan.T3, H.scan.Q);
	H.scan.T3.per_wg *= 2u; H.scan.T3.slice_cap = J.pair_slice_cap; H.scan.T3.n_irr_wg = (H.scan.T3.n_irr_wg + 1u)/2u;
	H.scan.cand_fwd = ctx->d_cand_fwd; H.scan.cand_floor = ctx->d_cand_floor; H.scan.sink = H.sink;
	H.scan.Z = group_clear(H.T, &J.fa, H.sink, true);
	H.post = post_row_args(ctx, S, H.sink, &J.fa, J.seq);
	return PCR_OK;
}

// Stage B of two passes at once (launcher thread): each prepared, the two joint launches, each one's bookkeeping.
int run_pass_pair(PassJob &JA, PassJob &JB)
{
	PairHalf H[2];
	H[0].ctx = JA.ctx; H[0].J = &JA; H[1].ctx = JB.ctx; H[1].J = &JB;
	int rc;
	for(PairHalf &h : H){
		h.S = &h.ctx->sets[h.J->which];
		if((rc = prepare_half(h)) != PCR_OK) return rc;
	}
	pcr_ctx *const ctx = JA.ctx;
	HostTimer timer(ctx, 2);
	const uint32_t Gx = seed3_grid(ctx)/2;
	const size_t dyn3 = std::max(seed3_lds(H[0].scan.T3), seed3_lds(H[1].scan.T3));
	if(!ctx->s3_pair_attr_set){
		HIP_TRY(hipFuncSetAttribute((const void *)k_seed3_pair<S3_WG_THREADS>, hipFuncAttributeMaxDynamicSharedMemorySize, 128*1024));
		ctx->s3_pair_attr_set = true;
	}
	const uint32_t Px = (std::max(H[0].S->n, H[1].S->n) + 7u)/8u;
	if(ctx->debug_log) fprintf(stderr, "[pcramp] paired launch: passes %u + %u, scan grid %u x 2 (irregular workgroups %u + %u, slice_cap' %u + %u, %zu B of LDS), tail grid %u x 2\n",
		JA.seq, JB.seq, Gx, H[0].scan.T3.n_irr_wg, H[1].scan.T3.n_irr_wg, H[0].scan.T3.slice_cap, H[1].scan.T3.slice_cap, dyn3, Px);
	hipLaunchKernelGGL(k_seed3_pair<S3_WG_THREADS>, dim3(Gx, 2), dim3(S3_WG_THREADS), dyn3, ctx->stream, H[0].scan, JA.pair_W, H[1].scan, JB.pair_W);
	HIP_TRY(hipGetLastError());
	hipLaunchKernelGGL(k_post_pair<8>, dim3(Px, 2), dim3(64*8), 0, ctx->stream, H[0].post, H[1].post);
	HIP_TRY(hipGetLastError());
	for(PairHalf &h : H){
		h.S->ctrl_clean = true; h.S->touched_from_seg = true;          // (as fused_tail)
		h.J->fa.posted = true; h.S->touched_built = false;
		pass_enqueued(*h.S, POST_CAP);
	}
	return PCR_OK;
}

void fill_job(pcr_ctx *ctx, PassJob &J, pcr_set which, int optimize_5, int optimize_3, float threshold, uint32_t min_oligo_length, bool async, const FusedAmp *fa)
{
	J.ctx = ctx; J.which = (int)which; J.opt5 = optimize_5; J.opt3 = optimize_3; J.thr = threshold; J.min_len = min_oligo_length; J.async = async;
	J.has_fa = fa != nullptr;
	if(fa){ J.fa = *fa; J.args = *fa->a; J.fa.a = &J.args; }            // (the job outlives the call: it keeps the arguments by value)
}

// Before a pass is launched from the calling thread: every pass queued on the handle's stream -- by whichever handle; the launcher
// thread may be holding one for a partner -- is launched first, so that the passes of a stream reach it in call order.
void quiesce_stream(pcr_ctx *ctx);

// pcr_select_words proper, and the inline pcr_screen_device pass: stage A and stage B on the calling thread, with a job on the
// stack.  fa: in/out (staged, posted, pub_*).
int select_impl(pcr_ctx *ctx, pcr_set which, const pcr_pair *pairs, uint32_t n_pairs, int optimize_5, int optimize_3,
	float threshold, uint32_t min_oligo_length, uint64_t *n_entries_out, bool async, FusedAmp *fa = nullptr)
{
	if(!ctx || (n_pairs && !pairs)){ g_err = "pcr_select_words: bad argument"; return PCR_ERR_ARG; }
	if(min_oligo_length < 1 || min_oligo_length > 32){ g_err = "pcr_select_words: min_oligo_length must be in [1,32]"; return PCR_ERR_ARG; }
	HIP_TRY(hipSetDevice(ctx->device));
	if(n_entries_out) *n_entries_out = 0;
	assert(ctx->lq_client.queued.load() == 0);           // inline: every caller came through DRAIN or flush_launcher
	quiesce_stream(ctx);
	PassJob J;
	fill_job(ctx, J, which, optimize_5, optimize_3, threshold, min_oligo_length, async, fa);
	J.ctrl_was_clean = begin_pass(ctx->sets[which]); J.begun = true;
	int rc = plan_pass(ctx, J, pairs, n_pairs);
	if(rc == PCR_OK) rc = run_pass(ctx, J, n_entries_out);
	if(fa){ const pcr_amplify_args *a = fa->a; *fa = J.fa; fa->a = a; }
	return rc;
}

// ---- the launcher thread of a stream (pcr_launch_queue.hpp) and the handles' side of it

// One per (device, stream), shared by every handle created on that stream and counted by them: the passes of several handles
// on one stream (an optimiser screens target, background and multiplex sets in turn, into buffers it alternates) must reach the
// stream in call order.  Made by the first pipelined pass; stopped and joined when its last handle is destroyed.
struct Launcher {
	int device; hipStream_t stream; unsigned refs = 0;
	cpu_set_t near; bool have_near = false;     // where the thread should run: see near_cpus()
	// the passes this thread has put on the stream and not yet seen published (launcher thread; forget_handle under the lock)
	struct InFlight { const pcr_ctx *ctx; const PassMail *slot; uint32_t seq; };
	std::mutex inflight_m; std::vector<InFlight> inflight;
	pcrq::LaunchQueue q;
	Launcher(int dev, hipStream_t st, unsigned spin_us);
	void forget_published()                          // (under inflight_m)
	{
		inflight.erase(std::remove_if(inflight.begin(), inflight.end(), [](const InFlight &f){
			const uint32_t v = __atomic_load_n((const uint32_t *)&f.slot->seq, __ATOMIC_ACQUIRE);
			return v >= f.seq && (v - f.seq) % pcr_ctx::MAIL_RING == 0; }), inflight.end());
	}
	void launched(const PassJob &J)
	{
		std::lock_guard<std::mutex> lk(inflight_m);
		// (nobody asks for the backlog of a stream that never holds a pass: the list must not grow there.  A handle has at most
		// MAIL_RING passes unpublished, so what is left beyond a few rings' worth belongs to a stream that has stopped publishing)
		if(inflight.size() >= 4*pcr_ctx::MAIL_RING){ forget_published(); if(inflight.size() >= 4*pcr_ctx::MAIL_RING) inflight.erase(inflight.begin()); }
		inflight.push_back(InFlight{ J.ctx, J.ctx->mail.host + (J.seq % pcr_ctx::MAIL_RING), J.seq });
	}
	// passes on the stream whose tail has not started (k_post publishes at its start): the GPU's backlog
	size_t backlog()
	{
		std::lock_guard<std::mutex> lk(inflight_m);
		forget_published();
		return inflight.size();
	}
	void forget_handle(const pcr_ctx *ctx)            // pcr_destroy, after the handle's flush: its mailbox is about to go
	{
		std::lock_guard<std::mutex> lk(inflight_m);
		inflight.erase(std::remove_if(inflight.begin(), inflight.end(), [&](const InFlight &f){ return f.ctx == ctx; }), inflight.end());
	}
};
// A lone pairable pass is held at most this long (the backlog rule or a flush end the hold long before; PCRAMP_PAIR=force and a
// stream that has stopped publishing after a device error are what it bounds).
constexpr unsigned PAIR_HOLD_CAP_US = 20000;
std::mutex g_launchers_m;
std::vector<Launcher *> g_launchers;

PassJob *acquire_job(pcr_ctx *ctx)
{
	PassJob *J = nullptr;
	{
		std::lock_guard<std::mutex> lk(ctx->job_m);
		if(!ctx->job_free.empty()){ J = ctx->job_free.back(); ctx->job_free.pop_back(); }
	}
	if(!J){ J = new PassJob(); ctx->job_all.push_back(J); }
	return J;
}
void release_job(pcr_ctx *ctx, PassJob *J)
{
	J->reset();
	std::lock_guard<std::mutex> lk(ctx->job_m);
	ctx->job_free.push_back(J);
}
void free_jobs(pcr_ctx *ctx)
{
	for(PassJob *J : ctx->job_all) delete J;
	ctx->job_all.clear(); ctx->job_free.clear();
}

// After its last job the thread spins on the queue this long before it blocks: a pass arrives every 15-25 us while a caller
// screens, and a condition-variable wake-up costs more than that.  Bounded: the process has 16 cores, and an idle handle must
// cost none (PCRAMP_LAUNCH_SPIN_US for the A/B).
constexpr unsigned LAUNCH_SPIN_US = 200;

// A CPU list of sysfs ("0-7,64-71") as a set.
bool read_cpu_list(const std::string &path, cpu_set_t &set)
{
	CPU_ZERO(&set);
	FILE *f = fopen(path.c_str(), "r");
	if(!f) return false;
	char buf[4096]; const bool got = fgets(buf, sizeof(buf), f) != nullptr;
	fclose(f);
	if(!got) return false;
	for(const char *p = buf;*p && *p != '\n';){
		char *e; const long a = strtol(p, &e, 10);
		if(e == p) return false;
		long b = a;
		if(*e == '-'){ p = e + 1; b = strtol(p, &e, 10); if(e == p) return false; }
		for(long c = a;c <= b && c < CPU_SETSIZE;++c) CPU_SET((int)c, &set);
		p = (*e == ',') ? e + 1 : e;
	}
	return true;
}
// The CPUs the launcher thread should run on: those that share the last-level cache with the CPU the caller is on, without the
// caller's own core.  Every pass hands some 25 KB of freshly written tables from the caller's thread to the launcher's; with the
// two threads on different sockets or cache domains those lines cross the fabric one by one and stage A ran 2-3x slower than
// inline.  false (no pinning): not Linux's sysfs, or nothing left after the process's own affinity mask.
bool near_cpus(cpu_set_t &out)
{
	const int cpu = sched_getcpu();
	if(cpu < 0) return false;
	const std::string base = "/sys/devices/system/cpu/cpu" + std::to_string(cpu);
	cpu_set_t llc, core, allowed;
	if(!read_cpu_list(base + "/cache/index3/shared_cpu_list", llc)) return false;
	if(!read_cpu_list(base + "/topology/thread_siblings_list", core)) CPU_ZERO(&core);
	CPU_SET(cpu, &core);
	if(sched_getaffinity(0, sizeof(allowed), &allowed) != 0) return false;
	CPU_ZERO(&out);
	for(int c = 0;c < CPU_SETSIZE;++c){ if(CPU_ISSET(c, &llc) && CPU_ISSET(c, &allowed) && !CPU_ISSET(c, &core)) CPU_SET(c, &out); }
	return CPU_COUNT(&out) > 0;
}

Launcher::Launcher(int dev, hipStream_t st, unsigned spin_us) : device(dev), stream(st),
	q([this](void *job, std::string &err) -> int {
		PassJob &J = *(PassJob *)job;
		assert(J.seq != 0 && J.ctx->launcher);
		if(J.ctx->debug_log) fprintf(stderr, "[pcramp] single launch: pass %u of handle %p (%s)\n", J.seq, (void *)J.ctx, pass_is_pairable(J.ctx, J) ? "pairable" : "not pairable");
		const int rc = run_pass(J.ctx, J, nullptr);
		if(rc != PCR_OK) err = g_err;                     // (this thread's: the handle's next call copies it into its own)
		else launched(J);
		return rc;
	},
	[](void *job){ PassJob *J = (PassJob *)job; release_job(J->ctx, J); },
	[this]{
		if(have_near) (void)pthread_setaffinity_np(pthread_self(), sizeof(near), &near);
		(void)hipSetDevice(device);
	},
	spin_us)
{
	const char *v = getenv("PCRAMP_LAUNCH_PIN");           // =0: leave the thread's placement to the scheduler (A/B)
	have_near = !(v && v[0] == '0') && near_cpus(near);
	// Pairs (run_pass_pair).  This thread is faster than the callers, so its queue is normally empty and the backlog sits in the
	// stream: a lone pairable pass is held only while the GPU still has two passes to start -- holding then costs nothing -- or,
	// with PCRAMP_PAIR=force, until something ends the hold (pcr_launch_queue.hpp).
	pcrq::LaunchQueue::Pairing pr;
	pr.holdable = [](void *job){ const PassJob &J = *(const PassJob *)job; return pass_is_pairable(J.ctx, J); };
	pr.may_hold = [this](void *job){ return ((const PassJob *)job)->ctx->pair_mode == 2 || backlog() >= 2; };
	pr.can_pair = [](void *a, void *b){
		PassJob &A = *(PassJob *)a, &B = *(PassJob *)b;
		const bool ok = passes_can_pair(A, B);
		if(!ok && A.ctx->debug_log) fprintf(stderr, "[pcramp] pass %u of handle %p does not pair with pass %u of handle %p behind it\n", A.seq, (void *)A.ctx, B.seq, (void *)B.ctx);
		return ok;
	};
	pr.run_pair = [this](void *a, void *b, std::string &err) -> int {
		PassJob &A = *(PassJob *)a, &B = *(PassJob *)b;
		const int rc = run_pass_pair(A, B);
		if(rc != PCR_OK) err = g_err;
		else{ launched(A); launched(B); }
		return rc;
	};
	pr.cap_us = PAIR_HOLD_CAP_US;
	q.set_pairing(std::move(pr));
}

Launcher *attach_launcher(pcr_ctx *ctx)
{
	if(ctx->launcher) return ctx->launcher;
	std::lock_guard<std::mutex> lk(g_launchers_m);
	for(Launcher *L : g_launchers){ if(L->device == ctx->device && L->stream == ctx->stream){ ++L->refs; return ctx->launcher = L; } }
	unsigned spin = LAUNCH_SPIN_US;
	if(const char *v = getenv("PCRAMP_LAUNCH_SPIN_US")) spin = (unsigned)std::min<unsigned long>(strtoul(v, nullptr, 0), 10000ul);
	Launcher *L = new Launcher(ctx->device, ctx->stream, spin);
	if(ctx->debug_log || ctx->timing) fprintf(stderr, "[pcramp] launcher thread for stream %p: caller on cpu %d, launcher %s (%d cpus), spin %u us\n", (void *)ctx->stream,
		sched_getcpu(), L->have_near ? "pinned beside it" : "not pinned", L->have_near ? CPU_COUNT(&L->near) : 0, spin);
	L->refs = 1;
	g_launchers.push_back(L);
	return ctx->launcher = L;
}
// pcr_destroy, after the handle's flush
void detach_launcher(pcr_ctx *ctx)
{
	Launcher *L = ctx->launcher;
	if(!L) return;
	ctx->launcher = nullptr;
	L->forget_handle(ctx);
	{
		std::lock_guard<std::mutex> lk(g_launchers_m);
		if(--L->refs) return;
		g_launchers.erase(std::find(g_launchers.begin(), g_launchers.end(), L));
	}
	L->q.stop();                                          // joins the thread
	delete L;
}

void quiesce_stream(pcr_ctx *ctx)
{
	if(ctx->launcher){ ctx->launcher->q.wait_empty(); return; }
	std::lock_guard<std::mutex> lk(g_launchers_m);       // (a handle that has not pipelined a pass yet: the stream's launcher, if another handle made one)
	for(Launcher *L : g_launchers){ if(L->device == ctx->device && L->stream == ctx->stream){ L->q.wait_empty(); return; } }
}

// Wait for the handle's queued passes to be launched.  One of them failed: its error comes back here, once, with the message in
// this thread's g_err; the passes queued behind it were dropped, and none of them stays pending.
int flush_launcher(pcr_ctx *ctx)
{
	if(!ctx->launcher) return PCR_OK;
	ctx->launcher->q.flush(&ctx->lq_client);
	int code; std::string msg; uint32_t seq;
	if(!ctx->lq_client.take_error(code, msg, seq)) return PCR_OK;
	std::vector<pcr_ctx::Pending> &pd = ctx->pending;
	pd.erase(std::remove_if(pd.begin(), pd.end(), [&](const pcr_ctx::Pending &q){ return (int32_t)(q.seq - seq) >= 0; }), pd.end());
	g_err = msg;
	return code;
}

// pcr_screen_device proper.  By default the pass is pipelined: this thread plans it (stage A) and hands it to the stream's
// launcher thread (stage B), which may still be staging and launching the previous one.  A pass whose planning or launch needs
// more than that -- the first over a set (it builds the index), first-form tables, shift candidates, a tail that is not fused --
// flushes the queue and runs inline, as every pass does with PCRAMP_LAUNCH_THREAD=0.
int screen_pass(pcr_ctx *ctx, pcr_set which, const pcr_pair *pairs, uint32_t n_pairs, int optimize_5, int optimize_3,
	float select_threshold, uint32_t min_oligo_length, const pcr_amplify_args *args, uint64_t *d_bits_fr, uint64_t *d_bits_rf)
{
	if(min_oligo_length < 1 || min_oligo_length > 32){ g_err = "pcr_select_words: min_oligo_length must be in [1,32]"; return PCR_ERR_ARG; }
	int rc;
	if(ctx->lq_client.poisoned.load(std::memory_order_acquire) && (rc = flush_launcher(ctx)) != PCR_OK) return rc;
	HIP_TRY(hipSetDevice(ctx->device));
	SeqSet &S = ctx->sets[which];
	FusedAmp fa; fa.pairs = pairs; fa.n_pairs = n_pairs; fa.a = args; fa.d_fr = d_bits_fr; fa.d_rf = d_bits_rf;
	PassJob *J = acquire_job(ctx);
	fill_job(ctx, *J, which, optimize_5, optimize_3, select_threshold, min_oligo_length, true, &fa);
	bool inline_pass = !ctx->launch_thread || !plans_without_device_work(ctx, S, optimize_5, optimize_3, min_oligo_length);
	if(inline_pass){
		if((rc = flush_launcher(ctx)) != PCR_OK){ release_job(ctx, J); return rc; }
		J->ctrl_was_clean = begin_pass(S); J->begun = true;
	}
	rc = plan_pass(ctx, *J, pairs, n_pairs);
	if(rc == PCR_OK && !inline_pass && !pass_is_pipelinable(ctx, *J)){
		inline_pass = true;
		rc = flush_launcher(ctx);
	}
	if(rc != PCR_OK){
		if(!J->begun){ (void)flush_launcher(ctx); (void)begin_pass(S); }      // (a failed plan leaves the set as it always has: without a DB)
		release_job(ctx, J);
		return rc;
	}
	pcr_ctx::Pending p;
	if(!ctx->pair_pool.empty()){ p.pairs.swap(ctx->pair_pool.back()); ctx->pair_pool.pop_back(); }   // (storage of a drained pass: no allocation per pass)
	p.which = (int)which; p.pairs.assign(pairs, pairs + n_pairs); p.opt5 = optimize_5; p.opt3 = optimize_3;
	p.thr = select_threshold; p.min_len = min_oligo_length; p.args = *args; p.d_fr = d_bits_fr; p.d_rf = d_bits_rf;
	if(!inline_pass){
		Launcher *L = attach_launcher(ctx);
		p.seq = J->seq = ++ctx->mail_seq;
		J->fa.pairs = nullptr;                                          // (the caller's array: stage A is done with it)
		ctx->pending.push_back(std::move(p));
		++ctx->n_pipelined;
		L->q.push(&ctx->lq_client, J, J->seq);
		return PCR_OK;
	}
	assert(ctx->lq_client.queued.load() == 0);           // stage B on this thread: the launcher thread holds no pass of the handle
	if(ctx->debug_log) fprintf(stderr, "[pcramp] inline pass of handle %p\n", (void *)ctx);
	quiesce_stream(ctx);
	const uint32_t seq0 = ctx->mail_seq;
	rc = run_pass(ctx, *J, nullptr);
	if(rc == PCR_OK && !J->fa.posted) rc = amplify_launch(ctx, S, pairs, n_pairs, args, d_bits_fr, d_bits_rf, &J->fa);
	release_job(ctx, J);
	if(rc != PCR_OK) return rc;
	if(ctx->mail_seq != seq0){                                        // a pass was enqueued (not the empty-input shortcut)
		p.seq = ctx->mail_seq;
		ctx->pending.push_back(std::move(p));
	}
	return PCR_OK;
}

// Look at the counters of the passes pcr_screen_device enqueued.  A pass whose buckets overflowed produced
// an incomplete DB (and so possibly incomplete amplification bits): grow the buckets and replay it and
// everything enqueued after it, synchronously, into the same output buffers.
int drain(pcr_ctx *ctx)
{
	{ const int frc = flush_launcher(ctx); if(frc != PCR_OK) return frc; }
	if(ctx->pending.empty()) return PCR_OK;
	std::vector<pcr_ctx::Pending> pend;
	pend.swap(ctx->pending);
	// however this returns: the drained passes' pair lists, and the list of passes itself, keep their storage for the next ones
	struct Recycle {
		pcr_ctx *ctx; std::vector<pcr_ctx::Pending> &pend;
		~Recycle()
		{
			for(pcr_ctx::Pending &q : pend){ if(ctx->pair_pool.size() < pcr_ctx::MAIL_RING) ctx->pair_pool.push_back(std::move(q.pairs)); }
			pend.clear();
			if(ctx->pending.empty() && ctx->pending.capacity() < pend.capacity()) ctx->pending.swap(pend);
		}
	} recycle{ctx, pend};
	int rc;
	for(size_t i = 0;i < pend.size();++i){
		uint32_t c[4];
		if((rc = mail_wait(ctx, pend[i].seq, c)) != PCR_OK) return rc;
		SeqSet &S = ctx->sets[pend[i].which];
		if(!(c[0] & 1u)){
			if(c[3] == N_TOUCHED_UNKNOWN_DEV){ S.n_touched = N_TOUCHED_UNKNOWN; S.n_entries = 1; }
			else{ S.n_touched = c[3]; S.n_entries = c[3] ? 1 : 0; }
			continue;
		}
		uint32_t want = S.bucket_cap*2;
		while(want < c[2] && want < MAX_BUCKET_CAP_GLOBAL) want *= 2;
		S.bucket_cap = std::min(want, MAX_BUCKET_CAP_GLOBAL);
		for(size_t j = i;j < pend.size();++j){
			const pcr_ctx::Pending &q = pend[j];
			if((rc = select_impl(ctx, (pcr_set)q.which, q.pairs.data(), (uint32_t)q.pairs.size(), q.opt5, q.opt3, q.thr, q.min_len, nullptr, false)) != PCR_OK) return rc;
			if((rc = amplify_launch(ctx, ctx->sets[q.which], q.pairs.data(), (uint32_t)q.pairs.size(), &q.args, q.d_fr, q.d_rf)) != PCR_OK) return rc;
		}
		break;
	}
	return PCR_OK;
}

} // namespace
