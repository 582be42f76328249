// The seed lists of a screen pass (pcrseed::list_seeds and pcrseed::plan_slices, pcramp_amd/csrc/pcr_seed_lists.hpp) on the CPU, as a
// stand-alone program: tests/test_seed_lists_host.py compiles it with -fsanitize=address,undefined and runs it.
//
// It carries a plain reference listing -- the loops the library ran before the listing moved into that header, written with
// std::vector per cache entry, resize / insert per orientation and a hash lookup per orientation, and the merge walk over the chunk
// list -- and requires BYTE EQUALITY of every output of the two on the same chain of passes: seeds, spans, prefix, the group arrays,
// masks, or_seed / or_plain, irr_off_mask, the return value, and of the slice plan start[], per_wg, slice_cap, n_chunks, n_irr_wg and
// its return value.  Both listings keep their caches over the whole chain, so what one pass leaves behind (entries, chunk counts per
// index generation, the memo) is what the next one finds.
//
// The chain (fixed-seed generator; synthetic run-length tables of 2^20 + 1 entries), once with the fold on and once with it off, each
// pass in both modes (third form: with a set; second form: without):
//   oligo lengths 18 ... 25 at thresholds 0.81, 0.9, 1.0 and 0.6 (orientations without a seed structure: or_plain); oligos with IUPAC
//   slots; a batch of one pair; a batch that closes several groups; the same batch twice (memo); that batch with oligos replaced, two
//   swapped, shortened, lengthened (stale memo); the cache-clear threshold crossed between two passes and in the middle of one; two
//   index generations alternating, then three more so that the fifth evicts a slot, then the first again; run tables that give
//   n_chunks == 0, a single seed with entries, and one run that dwarfs the rest; limits tightened until the listing returns false for
//   each of its reasons and until the slice plan does; the memo switched off.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unordered_map>
#include "../pcramp_amd/csrc/pcr_seed_lists.hpp"

using pcrhost::Planes;
using pcrhost::Candidate;
using pcrseed::Mask16;
using pcrseed::Limits;
using pcrseed::SetIndex;

static uint64_t g_rng = 0x452821E638D01377ull;
static uint32_t rnd(uint32_t n) { g_rng = g_rng*6364136223846793005ull + 1442695040888963407ull; return (uint32_t)((g_rng >> 33) % n); }
static int g_fail = 0;
static unsigned long long g_passes = 0, g_seeds = 0, g_plain = 0, g_false = 0, g_multi_group = 0, g_slices_false = 0, g_zero_chunks = 0;

#define CHECK(c, ...) do{ if(!(c)){ printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); if(++g_fail > 20) exit(1); } }while(0)

// ---------------------------------------------------------------------------------------------------------------------------------
// The reference: the listing as it stood, one std::vector per list and per cache entry.
namespace ref {

struct Key { uint32_t a, c, g, t, floor_; bool operator==(const Key &o) const { return a == o.a && c == o.c && g == o.g && t == o.t && floor_ == o.floor_; } };
struct KeyHash { size_t operator()(const Key &k) const { uint64_t h = 1469598103934665603ull; for(uint32_t v : {k.a, k.c, k.g, k.t, k.floor_}){ h ^= v; h *= 1099511628211ull; } return (size_t)h; } };
struct Entry2 { std::vector<uint32_t> seeds; uint32_t off_mask; bool seedable; Mask16 mask; };
constexpr int CHUNK_SETS = 4;
struct Chunks { uint64_t gen = 0; uint32_t total = 0; std::vector<uint32_t> run; };
struct Entry3 : Entry2 { std::vector<uint8_t> spans; Chunks chunks[CHUNK_SETS]; uint32_t next_slot = 0; };
struct Ctx {
	std::unordered_map<Key, Entry2, KeyHash> s2_cache; std::unordered_map<Key, Entry3, KeyHash> s3_cache;
	std::vector<pcrhost::Seed> s2_tmp; std::vector<pcrhost::FoldSeed> s3_tmp;
	size_t clear_above = 16384; bool s3_next = true;
};
struct Lists {
	std::vector<uint32_t> s2_seeds; std::vector<Mask16> s2_masks;
	std::vector<uint32_t> s2_group_end, s2_group_offmask, s2_group_or, s2_group_nor;
	std::vector<uint32_t> s3_prefix; std::vector<uint8_t> s3_spans;
};

// slot k < 16 -> bit 2k, slot 16 + k -> bit 2k + 1
static uint32_t interleave(uint32_t plane)
{
	uint32_t r = 0;
	for(int k = 0;k < 16;++k){ if(plane & (1u << k)) r |= 1u << (2*k); if(plane & (1u << (16 + k))) r |= 1u << (2*k + 1); }
	return r;
}

static bool plan_seed2(Ctx *ctx, const Limits &lim, bool third_limits, Lists &L, const std::vector<Candidate> &cand, std::vector<uint32_t> &or_seed, std::vector<uint32_t> &or_plain,
	uint32_t &irr_off_mask, const SetIndex *S3)
{
	std::vector<uint32_t> &pf = L.s3_prefix;
	pf.clear();
	uint32_t pf_run = 0;
	const uint32_t n_or = 2*(uint32_t)cand.size();
	std::vector<uint32_t> &out = L.s2_seeds;
	out.clear(); L.s2_group_end.clear(); L.s2_group_offmask.clear(); L.s2_group_or.clear(); L.s2_group_nor.clear();
	irr_off_mask = 0;
	L.s2_masks.resize(n_or);
	if(ctx->s2_cache.size() > ctx->clear_above) ctx->s2_cache.clear();
	size_t group_begin = 0; uint32_t group_mask = 0, group_or0 = 0, group_last = 0;
	auto fits = [&](size_t n, uint32_t g_or){
		if(third_limits) return g_or <= lim.max_or && n <= lim.max_seeds;
		return g_or <= lim.max_or && n <= lim.max_seeds && lim.lds_fixed + 17*(size_t)g_or + 8*n <= lim.lds_budget;
	};
	auto mask_of = [](const Planes &m){ const Mask16 r = { interleave(m.a), interleave(m.c), interleave(m.g), interleave(m.t) }; return r; };
	std::vector<uint8_t> &spans = L.s3_spans;
	spans.clear();
	if(ctx->s3_cache.size() > ctx->clear_above) ctx->s3_cache.clear();
	for(uint32_t o = 0;o < n_or;++o){
		const Candidate &c = cand[o >> 1];
		const Planes &m = (o & 1u) ? c.rc : c.fwd;
		const Key key = {m.a, m.c, m.g, m.t, c.floor_};
		Entry3 *e3 = nullptr; const Entry2 *e2 = nullptr;
		if(S3){
			auto it = ctx->s3_cache.find(key);
			if(it == ctx->s3_cache.end()){
				Entry3 e; e.off_mask = 0;
				ctx->s3_tmp.clear(); ctx->s2_tmp.clear();
				e.seedable = pcrhost::orientation_index_seeds(m, c.floor_, ctx->s3_next, ctx->s3_tmp, ctx->s2_tmp);
				e.mask = mask_of(m);
				e.seeds.reserve(ctx->s3_tmp.size()); e.spans.reserve(ctx->s3_tmp.size());
				for(const pcrhost::FoldSeed &sd : ctx->s3_tmp){
					e.seeds.push_back((sd.code << 14) | ((uint32_t)sd.off << 9)); e.spans.push_back((uint8_t)(sd.lo | (sd.hi << 2))); e.off_mask |= 1u << sd.off;
				}
				it = ctx->s3_cache.emplace(key, std::move(e)).first;
			}
			e3 = &it->second; e2 = e3;
		}
		else{
			auto it = ctx->s2_cache.find(key);
			if(it == ctx->s2_cache.end()){
				Entry2 e; e.off_mask = 0;
				ctx->s2_tmp.clear();
				e.seedable = pcrhost::orientation_seeds(m, c.floor_, 0, ctx->s2_tmp, nullptr, 9);
				e.mask = mask_of(m);
				e.seeds.reserve(ctx->s2_tmp.size());
				for(const pcrhost::Seed &sd : ctx->s2_tmp){ e.seeds.push_back((sd.code << 14) | ((uint32_t)sd.off << 9)); e.off_mask |= 1u << sd.off; }
				it = ctx->s2_cache.emplace(key, std::move(e)).first;
			}
			e2 = &it->second;
		}
		const Entry2 &e = *e2;
		L.s2_masks[o] = e.mask;
		if(!e.seedable){ or_plain.push_back(o); continue; }
		or_seed.push_back(o);
		if(!fits(out.size() - group_begin + e.seeds.size(), o - group_or0 + 1)){
			if(!fits(e.seeds.size(), 1) || L.s2_group_end.size() + 1 >= lim.max_groups) return false;
			L.s2_group_end.push_back((uint32_t)out.size()); L.s2_group_offmask.push_back(group_mask); L.s2_group_or.push_back(group_or0); L.s2_group_nor.push_back(group_last - group_or0 + 1);
			group_begin = out.size(); group_mask = 0; group_or0 = o;
			if(S3){ pf.push_back(pf_run); pf_run = 0; }
		}
		group_last = o;
		const size_t at = out.size();
		out.resize(at + e.seeds.size());
		for(size_t k = 0;k < e.seeds.size();++k) out[at + k] = e.seeds[k] | (o - group_or0);
		if(S3){
			spans.insert(spans.end(), e3->spans.begin(), e3->spans.end());
			Chunks *ch = nullptr;
			for(Chunks &x : e3->chunks){ if(x.gen == S3->generation){ ch = &x; break; } }
			if(!ch){
				ch = &e3->chunks[e3->next_slot]; e3->next_slot = (e3->next_slot + 1u) % CHUNK_SETS;
				ch->run.resize(e.seeds.size());
				const uint32_t *const start = S3->start;
				uint32_t run = 0;
				for(size_t k = 0;k < e.seeds.size();++k){
					const uint32_t key4 = (e.seeds[k] >> 14) << 2, sp = e3->spans[k];
					ch->run[k] = run; run += (start[key4 + (sp >> 2) + 1u] - start[key4 + (sp & 3u)] + 63u) >> 6;
				}
				ch->total = run; ch->gen = S3->generation;
			}
			const size_t pa = pf.size();
			pf.resize(pa + ch->run.size());
			for(size_t k = 0;k < ch->run.size();++k) pf[pa + k] = pf_run + ch->run[k];
			pf_run += ch->total;
		}
		if(!(o & 1u)){ irr_off_mask |= e.off_mask; group_mask |= e.off_mask; }
	}
	L.s2_group_end.push_back((uint32_t)out.size()); L.s2_group_offmask.push_back(group_mask); L.s2_group_or.push_back(group_or0);
	L.s2_group_nor.push_back(or_seed.empty() ? 0u : group_last - group_or0 + 1);
	if(S3) pf.push_back(pf_run);
	return true;
}

} // namespace ref

constexpr uint32_t MAX_WG = 512;
struct Launch { struct { uint32_t start[MAX_WG + 1]; } W; uint32_t n_chunks, per_wg, slice_cap, n_irr_wg; };

namespace ref {
// the merge walk as it stood; `done`: the groups it reached (a false return stops at one)
static bool plan_seed3_slices(const Lists &PL, std::vector<Launch> &launch, uint32_t G_all, uint32_t seeds_per_turn, size_t lds_budget, bool with_irr, size_t &done)
{
	launch.resize(PL.s2_group_end.size());
	size_t g_begin = 0, g_prefix = 0;
	for(size_t g = 0;g < PL.s2_group_end.size();++g){
		done = g + 1;
		const uint32_t ns = PL.s2_group_end[g] - (uint32_t)g_begin;
		g_begin = PL.s2_group_end[g];
		const uint32_t *P = PL.s3_prefix.data() + g_prefix;
		g_prefix += (size_t)ns + 1;
		Launch &L = launch[g];
		L.n_irr_wg = with_irr ? std::min<uint32_t>((ns + seeds_per_turn - 1u)/seeds_per_turn, G_all/4u) : 0u;
		const uint32_t G = (G_all - L.n_irr_wg) & ~1u;
		L.n_chunks = P[ns]; L.per_wg = std::max<uint32_t>(1u, (L.n_chunks + G - 1u)/G); L.slice_cap = 2;
		if(ns == 0) continue;
		uint32_t at = 0;
		for(uint32_t w = 0;w <= G;++w){
			const uint64_t target = (uint64_t)w*L.per_wg;
			while(at + 1u < ns && P[at + 1u] <= target) ++at;
			L.W.start[w] = at;
		}
		for(uint32_t w = G + 1;w <= MAX_WG;++w) L.W.start[w] = at;
		for(uint32_t w = 0;w < G;++w) L.slice_cap = std::max(L.slice_cap, std::min(L.W.start[w + 1] + 2u, ns + 1u) - L.W.start[w]);
		if(17*(size_t)PL.s2_group_nor[g] + 9*(size_t)L.slice_cap + 64 > lds_budget) return false;
	}
	return true;
}
} // namespace ref

// ---------------------------------------------------------------------------------------------------------------------------------
// Inputs

static Planes planes_of_sets(const unsigned *sets)
{
	Planes p = {0, 0, 0, 0};
	for(int k = 0;k < 32;++k){
		if(sets[k] & 1u) p.a |= 1u << k;
		if(sets[k] & 2u) p.c |= 1u << k;
		if(sets[k] & 4u) p.g |= 1u << k;
		if(sets[k] & 8u) p.t |= 1u << k;
	}
	return p;
}

// an oligo of `size` bases centred as a 32-slot word holds it, with `iupac` slots of two or three bases
static Planes random_oligo(int size, int iupac)
{
	static const unsigned two[6] = {3, 5, 9, 6, 10, 12}, three[4] = {7, 11, 13, 14};
	unsigned sets[32];
	const int first = (32 - size)/2;
	for(int j = 0;j < 32;++j) sets[j] = (j >= first && j < first + size) ? 1u << rnd(4) : 0u;
	for(int i = 0;i < iupac;++i) sets[first + (int)rnd((uint32_t)size)] = (rnd(3) == 0) ? three[rnd(4)] : two[rnd(6)];
	return planes_of_sets(sets);
}

static Candidate candidate_of(const Planes &w, float thr, uint32_t index)
{
	Candidate c;
	c.fwd = w; c.rc = pcrhost::planes_revcomp(w);
	c.floor_ = (unsigned)((float)(unsigned)pcrhost::planes_size(w)*thr);
	c.base = index; c.shift = 0;
	return c;
}

// a batch of n_pairs pairs (two candidates each): lengths from [lo, hi]
static std::vector<Candidate> random_batch(uint32_t n_pairs, int lo, int hi, float thr, int iupac_every)
{
	std::vector<Candidate> cand;
	for(uint32_t i = 0;i < 2*n_pairs;++i){
		const int size = lo + (int)rnd((uint32_t)(hi - lo + 1));
		const int iupac = (iupac_every && i % (uint32_t)iupac_every == 0) ? 1 + (int)rnd(3) : 0;
		cand.push_back(candidate_of(random_oligo(size, iupac), thr, i));
	}
	return cand;
}

constexpr size_t N_KEYS = size_t(1) << 20;
struct RunTable {
	std::vector<uint32_t> start; uint64_t generation;
	SetIndex index() const { const SetIndex s = { start.data(), generation }; return s; }
};
static uint64_t g_generations = 0;
// runs of 0 ... max_run entries per 10-gram key (a third of the keys empty)
static RunTable random_table(uint32_t max_run)
{
	RunTable T; T.start.resize(N_KEYS + 1); T.generation = ++g_generations;
	uint32_t at = 0;
	for(size_t k = 0;k < N_KEYS;++k){ T.start[k] = at; if(max_run && rnd(3) != 0) at += rnd(max_run + 1); }
	T.start[N_KEYS] = at;
	return T;
}
// every run empty but that of `key`, which has `len` entries
static RunTable single_run_table(uint32_t key, uint32_t len, uint32_t others)
{
	RunTable T; T.start.resize(N_KEYS + 1); T.generation = ++g_generations;
	uint32_t at = 0;
	for(size_t k = 0;k < N_KEYS;++k){ T.start[k] = at; at += (k == key) ? len : (others ? rnd(others + 1) : 0u); }
	T.start[N_KEYS] = at;
	return T;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// One pass through both listings, everything compared

struct Both {
	pcrseed::Lister Z; ref::Ctx R;
	pcrseed::SeedLists L[3]; ref::Lists RL;        // (three lists in rotation, as the passes of a handle rotate their jobs)
	std::vector<Launch> launch, ref_launch;
	unsigned turn = 0;
	explicit Both(bool fold) { R.s3_next = fold; }
	void clear_above(size_t n) { Z.clear_above = n; R.clear_above = n; }
};

template<class A, class B> static bool same(const A &a, const B &b)
{
	if(a.size() != b.size()) return false;
	return a.size() == 0 || memcmp(a.data(), b.data(), a.size()*sizeof(*a.data())) == 0;
}

static const Limits LIM2 = { 256, 12288, 45056 + 1024, 160*1024, 4096 };   // (the second form's launch: the fixed part of its LDS image taken as 44 KB)
static const Limits LIM3 = { 448, 1u << 16, 0, ~size_t(0), 4096 };

// returns the listing's return value
static bool pass(Both &B, const std::vector<Candidate> &cand, const RunTable *T, const char *what, const Limits *lim_in = nullptr, size_t slice_budget = 120*1024)
{
	const bool third = T != nullptr;
	const Limits lim = lim_in ? *lim_in : (third ? LIM3 : LIM2);
	SetIndex ix = { nullptr, 0 }; if(T) ix = T->index();
	pcrseed::SeedLists &L = B.L[B.turn++ % 3];
	std::vector<uint32_t> os, op, ros, rop; uint32_t om = 0xDEADBEEFu, rom = 0xDEADBEEFu;
	const bool ok = pcrseed::list_seeds(B.Z, lim, cand.data(), cand.size(), T ? &ix : nullptr, B.R.s3_next, L, os, op, om);
	const bool rok = ref::plan_seed2(&B.R, lim, third, B.RL, cand, ros, rop, rom, T ? &ix : nullptr);
	++g_passes;
	CHECK(ok == rok, "%s: returns %d, the reference %d", what, (int)ok, (int)rok);
	if(!ok || !rok){ ++g_false; return ok; }
	CHECK(same(L.s2_seeds, B.RL.s2_seeds), "%s: seeds differ (%zu / %zu)", what, L.s2_seeds.size(), B.RL.s2_seeds.size());
	CHECK(same(L.s3_spans, B.RL.s3_spans), "%s: spans differ (%zu / %zu)", what, L.s3_spans.size(), B.RL.s3_spans.size());
	CHECK(same(L.s3_prefix, B.RL.s3_prefix), "%s: prefix differs (%zu / %zu)", what, L.s3_prefix.size(), B.RL.s3_prefix.size());
	CHECK(same(L.s2_masks, B.RL.s2_masks), "%s: masks differ", what);
	CHECK(same(L.s2_group_end, B.RL.s2_group_end) && same(L.s2_group_offmask, B.RL.s2_group_offmask) && same(L.s2_group_or, B.RL.s2_group_or)
		&& same(L.s2_group_nor, B.RL.s2_group_nor), "%s: group arrays differ", what);
	CHECK(same(os, ros) && same(op, rop), "%s: or_seed / or_plain differ", what);
	CHECK(om == rom, "%s: irr_off_mask %08x / %08x", what, om, rom);
	if(third){
		CHECK(L.s3_prefix.size() == L.s2_seeds.size() + L.s2_group_end.size() && L.s3_spans.size() == L.s2_seeds.size(), "%s: the third form's sizes", what);
	}
	else CHECK(L.s3_prefix.size() == 0 && L.s3_spans.size() == 0, "%s: chunk lists without a set", what);
	g_seeds += L.s2_seeds.size(); g_plain += op.size();
	if(L.s2_group_end.size() > 1) ++g_multi_group;
	if(!third) return ok;
	for(int with_irr = 0;with_irr < 2;++with_irr){
		size_t done = 0;
		const bool sok = pcrseed::plan_slices(L, B.launch, 512u, 256u, MAX_WG, slice_budget, with_irr != 0);
		const bool rsok = ref::plan_seed3_slices(B.RL, B.ref_launch, 512u, 256u, slice_budget, with_irr != 0, done);
		CHECK(sok == rsok, "%s: the slice plan returns %d, the reference %d", what, (int)sok, (int)rsok);
		if(!sok) ++g_slices_false;
		CHECK(B.launch.size() == B.ref_launch.size(), "%s: launches", what);
		size_t g_begin = 0;
		for(size_t g = 0;g < done && g < B.launch.size();++g){
			const Launch &a = B.launch[g], &b = B.ref_launch[g];
			const uint32_t ns = L.s2_group_end[g] - (uint32_t)g_begin; g_begin = L.s2_group_end[g];
			CHECK(a.n_chunks == b.n_chunks && a.per_wg == b.per_wg && a.slice_cap == b.slice_cap && a.n_irr_wg == b.n_irr_wg,
				"%s: group %zu: n_chunks %u/%u per_wg %u/%u slice_cap %u/%u n_irr_wg %u/%u", what, g, a.n_chunks, b.n_chunks, a.per_wg, b.per_wg, a.slice_cap, b.slice_cap, a.n_irr_wg, b.n_irr_wg);
			if(ns) CHECK(memcmp(a.W.start, b.W.start, sizeof a.W.start) == 0, "%s: group %zu: start[] differs", what, g);   // (a group without seeds leaves start[] alone)
			if(a.n_chunks == 0) ++g_zero_chunks;
		}
	}
	return ok;
}

static void both_modes(Both &B, const std::vector<Candidate> &cand, const RunTable &T, const char *what)
{
	pass(B, cand, &T, what);
	pass(B, cand, nullptr, what);
}

static void chain(bool fold)
{
	Both B(fold);
	const RunTable TA = random_table(200), TB = random_table(40);
	// lengths 18 ... 25 at each threshold (0.6: k = 8 and more mismatching slots -- no seed structure)
	static const float thr[4] = {0.81f, 0.9f, 1.0f, 0.6f};
	for(int ti = 0;ti < 4;++ti){
		for(int size = 18;size <= 25;++size) both_modes(B, random_batch(3, size, size, thr[ti], 0), TA, "one length");
		both_modes(B, random_batch(20, 18, 25, thr[ti], 0), TA, "mixed lengths");
	}
	// seeded and unseeded orientations side by side (the floors differ per candidate)
	{
		std::vector<Candidate> mix = random_batch(12, 18, 25, 0.9f, 0);
		for(size_t i = 0;i < mix.size();i += 3) mix[i].floor_ = (unsigned)((float)(unsigned)pcrhost::planes_size(mix[i].fwd)*0.6f);
		both_modes(B, mix, TA, "seeded and unseeded");
	}
	both_modes(B, random_batch(16, 18, 25, 0.9f, 2), TA, "IUPAC slots");
	both_modes(B, random_batch(8, 18, 25, 0.81f, 3), TA, "IUPAC slots at 0.81");
	both_modes(B, random_batch(1, 20, 20, 0.9f, 0), TA, "one pair");
	both_modes(B, std::vector<Candidate>(), TA, "no pair");
	// the memo: the same batch twice, then with its oligos moved about
	std::vector<Candidate> cur = random_batch(50, 18, 25, 0.9f, 0);
	both_modes(B, cur, TA, "batch"); both_modes(B, cur, TA, "batch again");
	for(int rep = 0;rep < 3;++rep){
		for(int i = 0;i < 7;++i){ const uint32_t at = rnd((uint32_t)cur.size()); cur[at] = candidate_of(random_oligo(18 + (int)rnd(8), 0), 0.9f, at); }
		both_modes(B, cur, TA, "some replaced");
	}
	std::swap(cur[3], cur[40]); std::swap(cur[4], cur[5]);
	both_modes(B, cur, TA, "two swapped");
	{ std::vector<Candidate> fewer(cur.begin(), cur.begin() + 31); both_modes(B, fewer, TA, "shortened"); }
	{ std::vector<Candidate> more(cur); const std::vector<Candidate> x = random_batch(9, 18, 25, 0.9f, 0); more.insert(more.end(), x.begin(), x.end()); both_modes(B, more, TA, "lengthened"); }
	both_modes(B, cur, TA, "back to the batch");
	{ std::vector<Candidate> other(cur); for(Candidate &c : other) c.floor_ = (unsigned)((float)(unsigned)pcrhost::planes_size(c.fwd)*1.0f); both_modes(B, other, TA, "another threshold"); both_modes(B, cur, TA, "and back"); }
	// several groups in both modes (448 orientations / 12 288 seeds a launch)
	const std::vector<Candidate> big = random_batch(300, 18, 25, 0.9f, 0);
	both_modes(B, big, TA, "several groups"); both_modes(B, big, TA, "several groups again");
	CHECK(g_multi_group >= 4, "no batch closed a group");
	// the cache-clear threshold: crossed between two passes (the next pass starts empty and must not meet its memo), and in the middle of
	// one (the pass goes on above it, the next one clears)
	// (every listing looks at BOTH caches when it starts, so each cache is crossed by passes of its own mode)
	for(int mode = 0;mode < 2;++mode){
		const RunTable *const T = mode ? nullptr : &TA;
		B.clear_above((mode ? B.Z.second.map.size() : B.Z.third.map.size()) + 30);
		pass(B, cur, T, "below the threshold");
		pass(B, random_batch(20, 18, 25, 0.9f, 0), T, "crosses the threshold in the middle");
		CHECK((mode ? B.Z.second.map.size() : B.Z.third.map.size()) > B.Z.clear_above, "the threshold was not crossed");
		CHECK((mode ? B.R.s2_cache.size() : B.R.s3_cache.size()) > B.R.clear_above, "the reference's threshold was not crossed");
		pass(B, cur, T, "first pass above the threshold");
		CHECK((mode ? B.Z.second.map.size() : B.Z.third.map.size()) <= cur.size()*2, "the cache was not cleared");
		pass(B, cur, T, "after the clear");
		B.clear_above(16384);
	}
	B.clear_above(60);                                                                 // (less than a batch holds: every pass clears)
	for(int rep = 0;rep < 3;++rep) both_modes(B, cur, TA, "a clear every pass");
	B.clear_above(16384);
	// index generations: two alternating, then three more (the fifth takes the first one's slot), then the first again
	for(int rep = 0;rep < 3;++rep){ pass(B, cur, &TA, "generation A"); pass(B, cur, &TB, "generation B"); }
	const RunTable TC = random_table(3), TD = random_table(1000), TE = random_table(90);
	pass(B, cur, &TC, "generation C"); pass(B, cur, &TD, "generation D"); pass(B, cur, &TE, "generation E"); pass(B, cur, &TA, "generation A after its slot went");
	pass(B, cur, &TB, "generation B after that"); pass(B, big, &TE, "several groups, generation E");
	// run tables: nothing anywhere; entries under one seed only; one run that dwarfs the rest
	const RunTable T0 = random_table(0);
	pass(B, cur, &T0, "empty index"); pass(B, big, &T0, "empty index, several groups");
	CHECK(g_zero_chunks > 0, "no launch without chunks");
	std::vector<pcrhost::FoldSeed> fs; std::vector<pcrhost::Seed> tmp;
	CHECK(pcrhost::orientation_index_seeds(cur[7].fwd, cur[7].floor_, fold, fs, tmp) && !fs.empty(), "an oligo of the batch has no seeds");
	const uint32_t key = (fs[fs.size()/2].code << 2) + fs[fs.size()/2].lo;
	const RunTable T1 = single_run_table(key, 37, 0), TH = single_run_table(key, 5000000, 30);
	pass(B, cur, &T1, "one seed with entries"); pass(B, cur, &TH, "one run that dwarfs the rest"); pass(B, big, &TH, "the same, several groups");
	// false returns: an orientation beyond one launch; too many groups; and the slice plan's (a slice that does not fit)
	const unsigned long long false0 = g_false;
	{ Limits t = LIM3; t.max_seeds = 20; CHECK(!pass(B, cur, &TA, "an orientation beyond a launch", &t), "accepted"); }
	{ Limits t = LIM2; t.max_seeds = 20; CHECK(!pass(B, cur, nullptr, "an orientation beyond a launch, second form", &t), "accepted"); }
	{ Limits t = LIM2; t.lds_budget = t.lds_fixed + 17 + 8*20; CHECK(!pass(B, cur, nullptr, "an orientation beyond the LDS, second form", &t), "accepted"); }
	{ Limits t = LIM3; t.max_or = 8; t.max_groups = 3; CHECK(!pass(B, cur, &TA, "too many groups", &t), "accepted"); }
	{ Limits t = LIM3; t.max_or = 8; t.max_groups = 64; CHECK(pass(B, cur, &TA, "groups of eight orientations", &t), "refused"); }
	{ Limits t = LIM2; t.max_or = 5; t.max_groups = 64; CHECK(pass(B, cur, nullptr, "groups of five orientations, second form", &t), "refused"); }
	CHECK(g_false == false0 + 4, "false returns: %llu", g_false - false0);
	const unsigned long long sf0 = g_slices_false;
	pass(B, cur, &T1, "a slice beyond the LDS", nullptr, 17*(size_t)(2*cur.size()) + 64 + 9*10);
	CHECK(g_slices_false > sf0, "the slice plan accepted a slice beyond its budget");
	// the memo switched off: every orientation through the hash
	B.Z.use_memo = false;
	both_modes(B, cur, TA, "no memo"); both_modes(B, big, TB, "no memo, several groups");
}

int main()
{
	chain(true);
	const unsigned long long plain_on = g_plain;
	chain(false);
	CHECK(plain_on > 0 && g_plain > plain_on, "no orientation without a seed structure");
	printf("%llu passes (%llu returned false, %llu closed a group), %llu seeds listed, %llu orientations without a seed structure\n", g_passes, g_false, g_multi_group, g_seeds, g_plain);
	if(g_fail){ printf("%d failures\n", g_fail); return 1; }
	printf("seed lists ok\n");
	return 0;
}
