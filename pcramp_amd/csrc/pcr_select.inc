namespace {

inline uint32_t spread16(uint32_t v)               // bit i of the low half -> bit 2i
{
	v &= 0xFFFFu;
	v = (v | (v << 8)) & 0x00FF00FFu; v = (v | (v << 4)) & 0x0F0F0F0Fu;
	v = (v | (v << 2)) & 0x33333333u; return (v | (v << 1)) & 0x55555555u;
}

// The seeds of a pass for the second form of the seed scan: per orientation from the cache (derived on a miss), listed as
// code << 14 | slot offset << 9 | orientation WITHIN ITS GROUP, in groups of at most S2_MAX_OR whole orientations, each of which
// fits the LDS budget of one launch.  One launch per group: IUPAC primers expand to more 9-gram seeds than one launch holds
// (two launches of this form still beat the first form, 2 x ~65 vs 178 + 22 us at C5's shard), and the reference's default
// batch of 1 000 trial assays (pcramp.h:32) is 4 000 orientations = 16+ groups (r02 sent it to the first form with host-built
// tables: 21 ms per select_words on a C5 shard).  false: an orientation whose seeds alone exceed one launch.
constexpr uint32_t S2_MAX_GROUPS = 4096;
// S3 (optional): the set whose position index the third form will read -- the chunk list of every launch group (ctx->s3_prefix: the
// running number of 64-entry chunks of the group's seeds' runs, its total behind it) is made alongside, from chunk counts cached
// beside each oligo's seeds for the set last used.
bool plan_seed2(pcr_ctx *ctx, const std::vector<pcrhost::Candidate> &cand, std::vector<uint32_t> &or_seed, std::vector<uint32_t> &or_plain, uint32_t &irr_off_mask,
	const SeqSet *S3 = nullptr)
{
	std::vector<uint32_t> &pf = ctx->s3_prefix;
	pf.clear();
	uint32_t pf_run = 0;
	const uint32_t n_or = 2*(uint32_t)cand.size();
	std::vector<uint32_t> &out = ctx->s2_seeds;
	out.clear(); ctx->s2_group_end.clear(); ctx->s2_group_offmask.clear(); ctx->s2_group_or.clear(); ctx->s2_group_nor.clear();
	irr_off_mask = 0;
	ctx->s2_masks.resize(n_or);
	if(ctx->s2_cache.size() > 16384) ctx->s2_cache.clear();
	size_t group_begin = 0; uint32_t group_mask = 0, group_or0 = 0, group_last = 0;
	// the tables of a launch must fit one CU's LDS; the third form keeps only the masks and a slice of the lists there: more orientations
	// (9-bit ids) and as many seeds as the pass has -- plan_seed3_slices() checks its LDS need afterwards
	auto fits = [&](size_t n, uint32_t g_or){
		if(S3) return g_or <= S3_MAX_OR && n <= S3_MAX_SEEDS;
		return g_or <= S2_MAX_OR && n <= S2_MAX_SEEDS && sizeof(S2Shared) + 17*(size_t)g_or + 8*n + 1024 <= 160*1024;
	};
	for(uint32_t o = 0;o < n_or;++o){
		const pcrhost::Candidate &c = cand[o >> 1];
		const Planes &m = (o & 1u) ? c.rc : c.fwd;
		const pcr_ctx::S2Key key = {m.a, m.c, m.g, m.t, c.floor_};
		auto it = ctx->s2_cache.find(key);
		if(it == ctx->s2_cache.end()){
			pcr_ctx::S2Entry e; e.off_mask = 0;
			ctx->s2_tmp.clear();
			e.seedable = pcrhost::orientation_seeds(m, c.floor_, 0, ctx->s2_tmp, nullptr, S2_Q);
			// per orientation ONE 16-byte mask entry: the four base-set planes, slots 0..15 spread to the even bits (slot k -> bit 2k) and
			// slots 16..31 to the odd bits (slot 16 + k -> bit 2k + 1): both halves of a window are counted by one multiplexer pass
			// (s2_count) from one LDS read
			e.mask = make_uint4(spread16(m.a) | (spread16(m.a >> 16) << 1), spread16(m.c) | (spread16(m.c >> 16) << 1),
			                    spread16(m.g) | (spread16(m.g >> 16) << 1), spread16(m.t) | (spread16(m.t >> 16) << 1));
			e.seeds.reserve(ctx->s2_tmp.size());
			for(const pcrhost::Seed &sd : ctx->s2_tmp){ e.seeds.push_back((sd.code << 14) | ((uint32_t)sd.off << 9)); e.off_mask |= 1u << sd.off; }
			it = ctx->s2_cache.emplace(key, std::move(e)).first;
		}
		pcr_ctx::S2Entry &e = it->second;
		ctx->s2_masks[o] = e.mask;
		if(!e.seedable){ or_plain.push_back(o); continue; }
		or_seed.push_back(o);
		// the group spans orientations [group_or0, o]: unseedable ones in between only take an (unused) id
		if(!fits(out.size() - group_begin + e.seeds.size(), o - group_or0 + 1)){   // close the group, open the next at this orientation
			if(!fits(e.seeds.size(), 1) || ctx->s2_group_end.size() + 1 >= S2_MAX_GROUPS) return false;
			ctx->s2_group_end.push_back((uint32_t)out.size()); ctx->s2_group_offmask.push_back(group_mask); ctx->s2_group_or.push_back(group_or0); ctx->s2_group_nor.push_back(group_last - group_or0 + 1);
			group_begin = out.size(); group_mask = 0; group_or0 = o;
			if(S3){ pf.push_back(pf_run); pf_run = 0; }                                // the group's total; the next one starts at 0
		}
		group_last = o;
		const size_t at = out.size();
		out.resize(at + e.seeds.size());
		for(size_t k = 0;k < e.seeds.size();++k) out[at + k] = e.seeds[k] | (o - group_or0);
		if(S3){
			if(e.chunks_gen != S3->pix_generation){                                   // exclusive running chunk counts of the oligo's seeds in this set
				e.chunks.resize(e.seeds.size());
				uint32_t run = 0;
				for(size_t k = 0;k < e.seeds.size();++k){ e.chunks[k] = run; run += (S3->pix_count_h[e.seeds[k] >> 14] + 63u) >> 6; }
				e.chunks_total = run; e.chunks_gen = S3->pix_generation;
			}
			const size_t pa = pf.size();
			pf.resize(pa + e.chunks.size());
			for(size_t k = 0;k < e.chunks.size();++k) pf[pa + k] = pf_run + e.chunks[k];
			pf_run += e.chunks_total;
		}
		if(!(o & 1u)){ irr_off_mask |= e.off_mask; group_mask |= e.off_mask; }   // slot offsets at which forward seeds sit (irregular-word scan)
	}
	ctx->s2_group_end.push_back((uint32_t)out.size()); ctx->s2_group_offmask.push_back(group_mask); ctx->s2_group_or.push_back(group_or0);
	ctx->s2_group_nor.push_back(or_seed.empty() ? 0u : group_last - group_or0 + 1);
	if(S3) pf.push_back(pf_run);
	return true;
}

// Third form: the chunks of every launch group dealt to G workgroups in equal contiguous shares, and per workgroup the first seed of its
// share (a merge walk over the group's chunk list).  false: some group's largest slice does not fit the LDS (many seeds whose runs are
// empty side by side: tiny target sets) -- the caller plans again within the second form's limits.
constexpr size_t S3_LDS_BUDGET = 120*1024;
// 1024-thread workgroups, two per CU (512 threads x 4 per CU: within the spread of the repeated default, profiles/dbg/r03_ab_s3_grid.txt)
constexpr uint32_t S3_WG_THREADS = 1024;
uint32_t seed3_grid(const pcr_ctx *ctx) { return std::min<uint32_t>(2*ctx->n_cu, S3_MAX_WG); }
bool plan_seed3_slices(pcr_ctx *ctx, bool with_irr)
{
	const uint32_t G_all = seed3_grid(ctx), seeds_per_turn = 16u*(S3_WG_THREADS/64);
	ctx->s3_launch.resize(ctx->s2_group_end.size());
	size_t g_begin = 0, g_prefix = 0;
	for(size_t g = 0;g < ctx->s2_group_end.size();++g){
		const uint32_t ns = ctx->s2_group_end[g] - (uint32_t)g_begin;
		g_begin = ctx->s2_group_end[g];
		const uint32_t *P = ctx->s3_prefix.data() + g_prefix;                  // the group's chunk list, [ns + 1]
		g_prefix += (size_t)ns + 1;
		pcr_ctx::S3Launch &L = ctx->s3_launch[g];
		// the launch's first workgroups look the irregular words up (16 seeds per wave turn) and leave the chunks to the others: the two
		// chains of dependent loads then run side by side; at most a quarter of the launch
		L.n_irr_wg = with_irr ? std::min<uint32_t>((ns + seeds_per_turn - 1u)/seeds_per_turn, G_all/4u) : 0u;
		const uint32_t G = G_all - L.n_irr_wg;
		L.n_chunks = P[ns]; L.per_wg = std::max<uint32_t>(1u, (L.n_chunks + G - 1u)/G); L.slice_cap = 2;
		if(ns == 0) continue;
		uint32_t at = 0;
		for(uint32_t w = 0;w <= G;++w){
			const uint64_t target = (uint64_t)w*L.per_wg;
			while(at + 1u < ns && P[at + 1u] <= target) ++at;
			L.W.start[w] = at;
		}
		for(uint32_t w = G + 1;w <= S3_MAX_WG;++w) L.W.start[w] = at;
		for(uint32_t w = 0;w < G;++w) L.slice_cap = std::max(L.slice_cap, std::min(L.W.start[w + 1] + 2u, ns + 1u) - L.W.start[w]);
		if(17*(size_t)ctx->s2_group_nor[g] + 8*(size_t)L.slice_cap + 64 > S3_LDS_BUDGET) return false;
	}
	return true;
}

// The seeds of a pass for the first form with device-built tables: per orientation from the cache (8-gram seeds), listed as
// code | slot offset << 16 | orientation << 21.  When the lists exceed S1_MAX_SEEDS (low thresholds: hundreds of codes per
// orientation) the orientations with the longest lists go to the bit-sliced scan.
void plan_seed1(pcr_ctx *ctx, const std::vector<pcrhost::Candidate> &cand, std::vector<uint32_t> &or_seed, std::vector<uint32_t> &or_plain, uint32_t &irr_off_mask)
{
	const uint32_t n_or = 2*(uint32_t)cand.size();
	std::vector<uint32_t> &out = ctx->s1_seeds;
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
// one popcount per (window, orientation).  The planners fill ctx->s2_* / s3_* / s1_seeds, which the launches read.
int choose_scan_form(pcr_ctx *ctx, SeqSet &S, const std::vector<pcrhost::Candidate> &cand, int optimize_5, int optimize_3, uint32_t min_oligo_length, ScanPlan &P)
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
			worth = plan_seed2(ctx, cand, os, op, om, nullptr) && op.empty() && !os.empty();
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
		use_seed2 = plan_seed2(ctx, cand, or_seed, or_plain, P.irr_off_mask, want_seed3 ? &S : nullptr);
		if(want_seed3 && !(use_seed2 && or_plain.empty() && !or_seed.empty() && plan_seed3_slices(ctx, P.s3_with_irr))){
			// the third form will not take the pass (an unseeded candidate, or its lists do not fit): plan within the second form's limits
			or_seed.clear(); or_plain.clear();
			use_seed2 = plan_seed2(ctx, cand, or_seed, or_plain, P.irr_off_mask, nullptr);
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
		&& ctx->s3_prefix.size() == ctx->s2_seeds.size() + ctx->s2_group_end.size();
	if(use_seed2){ P.form = use_seed3 ? ScanForm::Seed3 : ScanForm::Seed2; P.n_seeds = ctx->s2_seeds.size(); }
	else if(no_shifts && !ctx->host_seed_tables && n_or <= S1_MAX_OR){      // first form, tables built by k_seed_tables
		plan_seed1(ctx, cand, or_seed, or_plain, P.irr_off_mask);
		P.form = ScanForm::Seed1Dev; P.n_seeds = ctx->s1_seeds.size();
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

// What the launches of a pass read on the device (stage_tables).
struct Scan2Staged { Scan2Tables T; const uint32_t *d_tab = nullptr, *d_bias = nullptr, *d_map = nullptr; };
struct StagedTables {
	SeedTables ST = {};
	Seed2Tables ST2 = {};
	const uint32_t *d_s3_prefix = nullptr;
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

int stage_tables(pcr_ctx *ctx, SeqSet &S, const std::vector<pcrhost::Candidate> &cand, const ScanPlan &P, FusedAmp *fa, bool async, bool ctrl_was_clean,
	HostTimer &timer, StagedTables &T)
{
	const uint32_t ncand = (uint32_t)cand.size(), n_or = 2*ncand;
	const bool seed2 = is_seed2(P.form), seed3 = P.form == ScanForm::Seed3;
	const bool build_tables = P.form == ScanForm::Seed1Dev;
	const HostSeedPlan &H = P.H;
	int rc;
	std::vector<uint4> hf(ncand), hr(ncand); std::vector<uint32_t> hfl(ncand);
	for(uint32_t c = 0;c < ncand;++c){
		hf[c] = make_uint4(cand[c].fwd.a, cand[c].fwd.c, cand[c].fwd.g, cand[c].fwd.t);
		hr[c] = make_uint4(cand[c].rc.a, cand[c].rc.c, cand[c].rc.g, cand[c].rc.t);
		hfl[c] = cand[c].floor_;
	}
	if(P.need_plain) build_scan2_tables(cand, P.or_plain, T.plain.T);
	if(P.need_seedset) build_scan2_tables(cand, P.or_seed, T.seedset.T);
	size_t bytes = ncand*(2*sizeof(uint4) + sizeof(uint32_t)) + 1024;
	bytes += (T.plain.T.tab.size() + T.plain.T.bias.size() + P.or_plain.size() + 256)*sizeof(uint32_t);
	bytes += (T.seedset.T.tab.size() + T.seedset.T.bias.size() + P.or_seed.size() + 256)*sizeof(uint32_t);
	bytes += (H.image.size() + H.heads.size() + H.multi.size() + 64)*sizeof(uint32_t);
	std::vector<uint4> &masks2 = ctx->s2_masks; std::vector<uint8_t> &floors2 = ctx->s2_floors;
	if(seed2){
		// (the mask entries come out of the per-oligo cache: plan_seed2)
		floors2.assign(((size_t)n_or + 15) & ~size_t(15), 0);
		for(uint32_t o = 0;o < n_or;++o) floors2[o] = (uint8_t)std::min<uint32_t>(cand[o >> 1].floor_, 255u);
		bytes += masks2.size()*sizeof(uint4) + floors2.size() + ctx->s2_seeds.size()*sizeof(uint32_t) + 512;
		if(seed3) bytes += ctx->s3_prefix.size()*sizeof(uint32_t) + 64;
	}
	if(build_tables) bytes += ctx->s1_seeds.size()*sizeof(uint32_t) + 256;
	// fused pass: the amplicon screen's oligo table travels with the scan tables, its result bitsets are
	// cleared by the same launch
	std::vector<OligoDev> ol;
	if(fa && fa->n_pairs){
		T.bits_bytes = (size_t)fa->n_pairs*((S.n + 63)/64)*sizeof(uint64_t);
		T.fuse = ((uintptr_t)fa->d_fr % 16 == 0) && ((uintptr_t)fa->d_rf % 16 == 0) && (T.bits_bytes % 16 == 0);
		if(T.fuse){ build_oligos(fa->pairs, fa->n_pairs, fa->a, ol); bytes += ol.size()*sizeof(OligoDev) + 64; }
	}
	timer.next(1);
	// the pass's control block (counters | per-sequence fills | segment ends)
	const uint64_t gen = S.ctrl.generation;
	if((rc = S.ctrl.ensure(8 + 2*(size_t)S.n + 4)) != PCR_OK) return rc;
	T.lean = ctx->direct_ok && async && T.fuse && seed2 && !P.or_seed.empty() && ctrl_was_clean && gen == S.ctrl.generation
		&& S.bucket_cap == POST_CAP && 2*fa->n_pairs <= 32*POST_MASK_WORDS;
	if(ctx->debug_log) fprintf(stderr, "[pcramp] staging: %s\n", T.lean ? "lean (tables written into device memory, no staging launch)" : "k_stage");
	Stager st(ctx);
	if((rc = T.lean ? st.begin_direct(bytes) : st.begin(bytes)) != PCR_OK) return rc;
	ctx->d_cand_fwd = st.put(hf.data(), ncand);
	ctx->d_cand_rc = st.put(hr.data(), ncand);
	ctx->d_cand_floor = st.put(hfl.data(), ncand);
	if(P.need_plain) stage_scan2(st, P.or_plain, T.plain);
	if(P.need_seedset) stage_scan2(st, P.or_seed, T.seedset);
	if(!H.image.empty()){
		T.ST.image = st.put(H.image.data(), H.image.size());
		T.ST.heads = st.put(H.heads.data(), H.heads.size());
		T.ST.multi = H.multi.empty() ? T.ST.heads : st.put(H.multi.data(), H.multi.size());
	}
	const uint32_t *d_s1_seeds = nullptr;
	if(build_tables){
		d_s1_seeds = st.put(ctx->s1_seeds.data(), ctx->s1_seeds.size());
		if((rc = ctx->s1_image.ensure(SEED_IMAGE_WORDS)) != PCR_OK) return rc;
		if((rc = ctx->s1_heads.ensure(2*(size_t)S1_MAX_SEEDS)) != PCR_OK) return rc;   // two words per distinct code
		if((rc = ctx->s1_multi.ensure(S1_MAX_SEEDS)) != PCR_OK) return rc;
		T.ST.image = ctx->s1_image.p; T.ST.heads = ctx->s1_heads.p; T.ST.multi = ctx->s1_multi.p; T.ST.flat = 1;
	}
	if(seed2){
		T.ST2.seeds = st.put(ctx->s2_seeds.data(), ctx->s2_seeds.size());
		T.ST2.masks = st.put(masks2.data(), masks2.size());
		T.ST2.floors = st.put(floors2.data(), floors2.size());
		T.ST2.n_seeds = (uint32_t)ctx->s2_seeds.size(); T.ST2.n_or = n_or;
		if(seed3) T.d_s3_prefix = st.put(ctx->s3_prefix.data(), ctx->s3_prefix.size());
	}
	// the staging launch also clears the control block and the result bitsets -- unless the pass is lean: then the tables
	// are already in device memory, the control block was left clean by the previous pass's tail and the first scan launch
	// clears the bitsets
	const size_t ctrl_bytes = (8 + 2*(size_t)S.n)*sizeof(uint32_t);
	if(T.fuse){
		fa->d_oligos = st.put(ol.data(), ol.size());
		fa->staged = true;
		if(T.lean) st.seal(ctx->mail_seq + 1);
		else if((rc = st.ship(S.ctrl.p, ctrl_bytes, fa->d_fr, T.bits_bytes, fa->d_rf, T.bits_bytes, ctx->mail_seq + 1)) != PCR_OK) return rc;
	}
	else if((rc = st.ship(S.ctrl.p, ctrl_bytes, nullptr, 0, nullptr, 0, ctx->mail_seq + 1)) != PCR_OK) return rc;
	if(build_tables){
		if((rc = ctx->s1_part.ensure(2*S1_GROUPS)) != PCR_OK) return rc;
		hipLaunchKernelGGL(k_seed_tables<false>, dim3(S1_GROUPS), dim3(S1_BUILD_THREADS), 0, ctx->stream, d_s1_seeds, (uint32_t)ctx->s1_seeds.size(),
			ctx->s1_part.p, ctx->s1_image.p, ctx->s1_heads.p, ctx->s1_multi.p);
		hipLaunchKernelGGL(k_seed_tables<true>, dim3(S1_GROUPS), dim3(S1_BUILD_THREADS), 0, ctx->stream, d_s1_seeds, (uint32_t)ctx->s1_seeds.size(),
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

// Third form: the launch of one seed group (its slices: plan_seed3_slices).
int launch_seed3_group(pcr_ctx *ctx, SeqSet &S, const Seed2Tables &Tg, const uint32_t *d_chunk_prefix, const pcr_ctx::S3Launch &L3, const IrrArgs2 &IA,
	const HitSink &sink, const S2Clear &Z)
{
	Seed3Tables T3; T3.seeds = Tg.seeds; T3.chunk_prefix = d_chunk_prefix; T3.masks = Tg.masks; T3.floors = Tg.floors;
	T3.n_seeds = Tg.n_seeds; T3.n_or = Tg.n_or; T3.or_base = Tg.or_base;
	T3.pix_first = S.pix_first.p; T3.pix_last = S.pix_last.p; T3.pix_ent = S.pix_ent.p;
	Seed3Set Q3 = { S.valid_d(), S.blk_info.p, S.blk_local.p, S.d_active.p };
	T3.n_chunks = L3.n_chunks; T3.per_wg = L3.per_wg; T3.slice_cap = L3.slice_cap;
	T3.n_irr_wg = IA.ix_first ? L3.n_irr_wg : 0u;           // (without the index the chunk workgroups are fewer than they could be: harmless)
	const size_t dyn3 = (size_t)Tg.n_or*sizeof(uint4) + 2*(size_t)T3.slice_cap*sizeof(uint32_t) + (((size_t)Tg.n_or + 15) & ~size_t(15)) + 16;
	if(!ctx->s3_attr_set){
		HIP_TRY(hipFuncSetAttribute((const void *)k_seed3<S3_WG_THREADS>, hipFuncAttributeMaxDynamicSharedMemorySize, 128*1024));
		ctx->s3_attr_set = true;
	}
	hipLaunchKernelGGL(k_seed3<S3_WG_THREADS>, dim3(seed3_grid(ctx)), dim3(S3_WG_THREADS), dyn3, ctx->stream, T3, Q3, IA, ctx->d_cand_fwd, ctx->d_cand_floor, sink, Z, L3.W);
	return PCR_OK;
}

// Second and third form: one launch per seed group (plan_seed2).  The second form runs persistent workgroups of 16 waves, one per
// CU (the tables they build take most of its LDS); the irregular words are taken by the same waves once their tiles are done.
int launch_seed_groups(pcr_ctx *ctx, SeqSet &S, const ScanPlan &P, const StagedTables &T, const FusedAmp *fa, const HitSink &sink)
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
		for(size_t g = 0, b = 0;g < ctx->s2_group_end.size();++g){ if((size_t)ctx->s2_group_end[g] - b > (size_t)sgrid.x*S2_THREADS) irr_by_index = false; b = ctx->s2_group_end[g]; }   // (a thread looks up at most one seed)
		if(irr_by_index && (rc = irr_index_usable(ctx, S, irr_by_index)) != PCR_OK) return rc;
	}
	uint32_t g_begin = 0, g_prefix = 0;
	bool first_launch = true;
	for(size_t g = 0;g < ctx->s2_group_end.size();++g){
		Seed2Tables Tg = T.ST2;
		const uint32_t or0 = ctx->s2_group_or[g], g_or = ctx->s2_group_nor[g];
		Tg.seeds = T.ST2.seeds + g_begin; Tg.n_seeds = ctx->s2_group_end[g] - g_begin;
		Tg.masks = T.ST2.masks + (size_t)or0; Tg.floors = T.ST2.floors + or0; Tg.n_or = g_or; Tg.or_base = or0;
		g_begin = ctx->s2_group_end[g];
		if(Tg.n_seeds == 0){ g_prefix += 1u; continue; }
		const size_t dyn = (size_t)g_or*sizeof(uint4) + (((size_t)g_or + 15) & ~size_t(15)) + 8*((size_t)Tg.n_seeds + 64) + 16;   // masks | floors | chain | head (each with 64 dummy slots)
		IrrArgs2 IA; IA.scan = S.irr_scan.p; IA.irr = S.irr.p; IA.n_live = P.n_live;
		IA.off_mask = ctx->s2_group_offmask[g];
		IA.exhaustive = first_launch ? 1u : 0u;                             // words holding IUPAC slots meet every candidate once, in the first launch
		IA.ix_first = IA.ix_last = IA.ix_words = nullptr; IA.min_cws = std::min<uint32_t>(P.min_len, 255u);
		if(!P.or_plain.empty()){                                            // unseeded candidates in the pass: every irregular word meets every candidate, once
			IA.off_mask = 0;
			if(!first_launch) IA.n_live = 0;
		}
		else if(irr_by_index){                                               // every candidate seeded, no IUPAC word in the set: the words come in through the index, by seed
			IA.ix_first = S.irx_first.p; IA.ix_last = S.irx_last.p; IA.ix_words = S.irx_words.p; IA.n_live = 0;
		}
		if(ctx->debug_log) fprintf(stderr, "[pcramp] k_seed2: %u workgroups, %u seeds of orientations %u..%u (group %zu of %zu), %zu + %zu B of LDS\n", sgrid.x, Tg.n_seeds,
			or0, or0 + g_or - 1, g + 1, ctx->s2_group_end.size(), sizeof(S2Shared), dyn);
		S2Clear Z = { nullptr, 0u, nullptr, 0u, nullptr };
		if(T.lean && first_launch){                                          // the first launch of a lean pass clears the result bitsets
			Z.z0 = (uint4 *)fa->d_fr; Z.z1 = (uint4 *)fa->d_rf; Z.n0 = Z.n1 = (uint32_t)(T.bits_bytes/16); Z.ctrl = sink.counters;
		}
		if(seed3){
			if((rc = launch_seed3_group(ctx, S, Tg, T.d_s3_prefix + g_prefix, ctx->s3_launch[g], IA, sink, Z)) != PCR_OK) return rc;
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
int launch_scans(pcr_ctx *ctx, SeqSet &S, const ScanPlan &P, const StagedTables &T, const FusedAmp *fa, const HitSink &sink)
{
	int rc = PCR_OK;
	const uint32_t ncand = sink.ncand;
	if(S.n_tiles){
		// events around the scan launches of every prof_stride-th pass (an event between two kernels costs a ~6 us queue bubble)
		ProfScope scan_prof(ctx, PCR_PROF_SCAN, ctx->prof && (ctx->prof_pass++ % ctx->prof_stride) == 0);
		if(P.need_plain && (rc = launch_scan2(ctx, S, T.plain.T, ncand, sink, T.plain.d_tab, T.plain.d_bias, nullptr, S.n_tiles, T.plain.d_map)) != PCR_OK) return rc;
		if(P.form == ScanForm::Popcount) rc = launch_popcount(ctx, S, sink);
		else if(is_seed1(P.form)) rc = launch_seed1(ctx, S, P, T, sink);
		else if(is_seed2(P.form)) rc = launch_seed_groups(ctx, S, P, T, fa, sink);
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
template<class K>
void launch_post(K kernel, uint32_t waves, pcr_ctx *ctx, SeqSet &S, const HitSink &sink, const FusedAmp *fa)
{
	hipLaunchKernelGGL(kernel, dim3((S.n + waves - 1)/waves), dim3(64*waves), 0, ctx->stream, sink.hits, sink.seq_count, sink.best, sink.ncand, S.planes.p,
		S.d_blk_off.p, S.irr.p, S.irr_off.p, S.db.p, S.d_seg_hi, sink.counters, sink.epoch, S.n,
		fa->d_oligos, fa->n_pairs, (2*fa->n_pairs + 31)/32, S.d_len.p, S.d_active.p, fa->a->amp_min, fa->a->amp_max,
		fa->a->ident_threshold, fa->a->use_taq_mama, fa->d_fr, fa->d_rf, (uint64_t)((S.n + 63)/64), ctx->mail_dev + (ctx->mail_seq % pcr_ctx::MAIL_RING), ctx->mail_seq);
}
int fused_tail(pcr_ctx *ctx, SeqSet &S, const HitSink &sink, FusedAmp *fa)
{
	++ctx->mail_seq;
	if(sink.cap == POST_CAP){
		// 8 waves per workgroup: 4 and 16 measured within the noise of 8 (profiles/dbg/r03_ab_post_waves.txt)
		launch_post(k_post<8>, 8, ctx, S, sink, fa);
		S.ctrl_clean = true; S.touched_from_seg = true;              // k_post zeroes the counters and fills it has read
	}
	else if(sink.cap == 128) launch_post(k_post_big<128, 4>, 4, ctx, S, sink, fa);
	else launch_post(k_post_big<256, 4>, 4, ctx, S, sink, fa);
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
		hipLaunchKernelGGL(k_publish, dim3(1), dim3(64), 0, ctx->stream, sink.counters, ctx->mail_dev + (ctx->mail_seq % pcr_ctx::MAIL_RING), ctx->mail_seq);
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

// pcr_select_words proper.  async: enqueue one attempt and return without looking at the counters
// (pcr_screen_device; the caller records the pass as pending).
int select_impl(pcr_ctx *ctx, pcr_set which, const pcr_pair *pairs, uint32_t n_pairs, int optimize_5, int optimize_3,
	float threshold, uint32_t min_oligo_length, uint64_t *n_entries_out, bool async, FusedAmp *fa = nullptr)
{
	if(!ctx || (n_pairs && !pairs)){ g_err = "pcr_select_words: bad argument"; return PCR_ERR_ARG; }
	if(min_oligo_length < 1 || min_oligo_length > 32){ g_err = "pcr_select_words: min_oligo_length must be in [1,32]"; return PCR_ERR_ARG; }
	HIP_TRY(hipSetDevice(ctx->device));
	SeqSet &S = ctx->sets[which];
	S.have_db = false; S.n_entries = 0;
	if(n_entries_out) *n_entries_out = 0;
	const bool ctrl_was_clean = S.ctrl_clean;         // left so by the fused tail of the previous pass over this set
	S.ctrl_clean = false; S.touched_from_seg = false;
	HostTimer timer(ctx, 0);
	if(ctx->timing) ++ctx->n_timed;
	std::vector<pcrhost::Candidate> cand;
	pcrhost::build_candidates((const uint64_t *)pairs, n_pairs, optimize_5 != 0, optimize_3 != 0, threshold, cand);
	const uint32_t ncand = (uint32_t)cand.size();
	if(S.n == 0 || ncand == 0){ S.have_db = true; S.n_touched = 0; return PCR_OK; }
	int rc;
	if((rc = ctx->best.ensure((size_t)S.n*ncand)) != PCR_OK) return rc;
	if(ctx->best.generation != ctx->best_seen){
		// fresh (uninitialised) storage: clear once; afterwards the epoch tag makes clearing unnecessary
		HIP_TRY(hipMemsetAsync(ctx->best.p, 0, ctx->best.cap*sizeof(uint32_t), ctx->stream));
		ctx->best_seen = ctx->best.generation; ctx->epoch = std::min(ctx->debug_epoch, EPOCH_LIMIT);
	}
	ScanPlan P;
	if((rc = choose_scan_form(ctx, S, cand, optimize_5, optimize_3, min_oligo_length, P)) != PCR_OK) return rc;
	if(ctx->debug_log) fprintf(stderr, "[pcramp] scan plan: form=%s, %u candidates, %zu seeded orientations (%zu seeds), %zu plain, %u/%u IUPAC tiles, %u-slot buckets\n",
		form_name(P.form), ncand, P.or_seed.size(), P.n_seeds, P.or_plain.size(), S.n_degen_tiles, S.n_tiles, S.bucket_cap);
	StagedTables T;
	if((rc = stage_tables(ctx, S, cand, P, fa, async, ctrl_was_clean, timer, T)) != PCR_OK) return rc;

	timer.next(2);
	uint32_t h_counters[4];
	if((rc = S.touched.ensure(S.n)) != PCR_OK) return rc;
	S.d_seg_hi = S.ctrl.p + 8 + S.n;
	for(int attempt = 0;;++attempt){
		const uint32_t cap = S.bucket_cap;
		const uint64_t n_slots = (uint64_t)S.n*cap;
		if(n_slots >= (uint64_t(1) << 32) || n_slots*(sizeof(Hit) + sizeof(DevEntry)) > (uint64_t(96) << 30)){
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
		HitSink sink; sink.best = ctx->best.p; sink.hits = ctx->hits.p; sink.seq_count = S.ctrl.p + 8;
		sink.counters = S.ctrl.p; sink.cap = cap; sink.ncand = ncand; sink.epoch = ctx->epoch;
		if((rc = launch_scans(ctx, S, P, T, fa, sink)) != PCR_OK) return rc;
		const bool fused = async && fa && fa->staged && (cap == POST_CAP || cap == 128 || cap == 256) && 2*fa->n_pairs <= 32*POST_MASK_WORDS;
		if((rc = fused ? fused_tail(ctx, S, sink, fa) : plain_tail(ctx, S, sink, async, fa)) != PCR_OK) return rc;
		if(async){
			S.db_cap = cap; S.n_slots = n_slots;
			S.n_touched = N_TOUCHED_UNKNOWN; S.n_entries = 1; S.have_db = true;
			return PCR_OK;
		}
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

// Look at the counters of the passes pcr_screen_device enqueued.  A pass whose buckets overflowed produced
// an incomplete DB (and so possibly incomplete amplification bits): grow the buckets and replay it and
// everything enqueued after it, synchronously, into the same output buffers.
int drain(pcr_ctx *ctx)
{
	if(ctx->pending.empty()) return PCR_OK;
	std::vector<pcr_ctx::Pending> pend;
	pend.swap(ctx->pending);
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
