// The seed lists of a screen pass as the caller's thread makes them (plain C++, no HIP): the per-orientation cache entry, the
// listing of a pass's seeds for the second and third forms of the seed scan, and the deal of a launch group's chunks to its
// workgroups.  pcr_select.inc (plan_seed2, plan_seed3_slices) calls these with the kernels' limits; tests/seed_lists_check.cpp
// runs them stand-alone against the loops they replaced.
//
// What the lists hold is described where the kernels read them (pcr_scan_seed2.inc, pcr_scan_seed3.inc).  How they are made:
//   * a cache entry keeps an orientation's seeds, span bytes and -- for the last CHUNK_SETS position-index generations -- the
//     exclusive chunk counts of its seeds in ONE allocation, so that listing it reads consecutive lines;
//   * a pass is listed in two sweeps: the first resolves every orientation's entry (a memo by position, then the hash, then a
//     derivation), forms the launch groups and knows every total; the lists are then sized once, WITHOUT value-initialising
//     them (RawBuf), and the second sweep writes seed | tag, prefix + run[k] and the span bytes through raw pointers.
#ifndef PCR_SEED_LISTS_HPP
#define PCR_SEED_LISTS_HPP

#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <new>
#include <unordered_map>
#include <vector>
#include "pcr_host.hpp"

namespace pcrseed {

using pcrhost::Planes;

// An orientation's mask entry as k_seed2 / k_seed3 read it: 16 bytes, the device's uint4.
struct Mask16 { uint32_t x, y, z, w; };

inline uint32_t spread16(uint32_t v)               // bit i of the low half -> bit 2i
{
	v &= 0xFFFFu;
	v = (v | (v << 8)) & 0x00FF00FFu; v = (v | (v << 4)) & 0x0F0F0F0Fu;
	v = (v | (v << 2)) & 0x33333333u; return (v | (v << 1)) & 0x55555555u;
}
// per orientation ONE 16-byte mask entry: the four base-set planes, slots 0..15 spread to the even bits (slot k -> bit 2k) and
// slots 16..31 to the odd bits (slot 16 + k -> bit 2k + 1): both halves of a window are counted by one multiplexer pass
// (s2_count) from one LDS read
inline Mask16 mask_of(const Planes &m)
{
	const Mask16 r = { spread16(m.a) | (spread16(m.a >> 16) << 1), spread16(m.c) | (spread16(m.c >> 16) << 1),
	                   spread16(m.g) | (spread16(m.g >> 16) << 1), spread16(m.t) | (spread16(m.t >> 16) << 1) };
	return r;
}

// A list that is sized without being value-initialised: resize() only moves the length (and keeps what lies below it when the
// storage grows), clear() keeps the storage.  For trivially copyable T.
template<class T> struct RawBuf {
	T *p = nullptr; size_t n = 0, cap = 0;
	RawBuf() {}
	RawBuf(const RawBuf &) = delete; RawBuf &operator=(const RawBuf &) = delete;
	~RawBuf() { free(p); }
	T *data() { return p; } const T *data() const { return p; }
	size_t size() const { return n; } bool empty() const { return n == 0; }
	T &operator[](size_t i) { return p[i]; } const T &operator[](size_t i) const { return p[i]; }
	void clear() { n = 0; }
	void resize(size_t want)
	{
		if(want > cap){
			const size_t c = want + want/2 + 64;
			T *q = (T *)realloc(p, c*sizeof(T));
			if(!q) throw std::bad_alloc();
			p = q; cap = c;
		}
		n = want;
	}
};

struct Key { uint32_t a, c, g, t, floor_; bool operator==(const Key &o) const { return a == o.a && c == o.c && g == o.g && t == o.t && floor_ == o.floor_; } };
struct KeyHash { size_t operator()(const Key &k) const { uint64_t h = 0x9E3779B97F4A7C15ull; for(uint32_t v : {k.a, k.c, k.g, k.t, k.floor_}){ h ^= v; h *= 0x100000001B3ull; h ^= h >> 29; } return (size_t)h; } };

// The exclusive running chunk counts of an oligo's seeds are kept for the sets whose position index has one of the last CHUNK_SETS
// generations, so that sets which alternate (the targets and backgrounds of a design iteration, a caller rotating over sets) do
// not recompute them pass after pass.
constexpr int CHUNK_SETS = 4;

// One orientation (oligo planes + floor) in the cache.  block: seeds[n] (code << 14 | off << 9), then for a third-form entry
// run[CHUNK_SETS][n] and spans[n] (lo | hi << 2) -- one allocation.
struct EntryHead {
	Mask16 mask = {0, 0, 0, 0}; uint32_t off_mask = 0, n = 0; bool seedable = false;
	uint32_t next_slot = 0, total[CHUNK_SETS] = {0, 0, 0, 0}; uint64_t gen[CHUNK_SETS] = {0, 0, 0, 0};
	uint32_t *block = nullptr;
};
struct Entry : EntryHead {
	Entry() {}
	Entry(Entry &&o) : EntryHead(o) { o.block = nullptr; }
	Entry(const Entry &) = delete; Entry &operator=(const Entry &) = delete;
	~Entry() { free(block); }
	const uint32_t *seeds() const { return block; }
	uint32_t *run(int slot) const { return block + (size_t)(1 + slot)*n; }
	const uint8_t *spans() const { return (const uint8_t *)(block + (size_t)(1 + CHUNK_SETS)*n); }
	void alloc(uint32_t n_seeds, bool third)
	{
		n = n_seeds;
		const size_t bytes = third ? (size_t)(1 + CHUNK_SETS)*n*sizeof(uint32_t) + n : (size_t)n*sizeof(uint32_t);
		block = (uint32_t *)malloc(bytes ? bytes : 1);
		if(!block) throw std::bad_alloc();
	}
};

// A cache of entries with the memo that goes with it: per orientation index the last pass's key and entry, so that an oligo which
// kept its place between two passes costs one 20-byte compare, not a hash lookup.  The memo points INTO the map (node-based:
// entries do not move), so the two are only ever cleared together.
struct Cache {
	struct Slot { Key key; Entry *e; };
	std::unordered_map<Key, Entry, KeyHash> map;
	std::vector<Slot> memo;
	void clear() { map.clear(); memo.clear(); }
};

// What the listing needs of the set whose position index the third form reads: start[] of its 10-gram runs (4^10 + 1 entries) and
// the index's generation (never 0).
struct SetIndex { const uint32_t *start; uint64_t generation; };

// The limits of one launch: g_or orientations and n seeds fit when g_or <= max_or, n <= max_seeds and
// lds_fixed + 17 g_or + 8 n <= lds_budget; at most max_groups - 1 groups.
struct Limits { uint32_t max_or, max_seeds; size_t lds_fixed, lds_budget; uint32_t max_groups; };

// Stage A's state for the listing: caller-thread only.
struct Lister {
	Cache second, third;                          // 9-gram lists | the third form's lists (folded, or plain with span A..T) under the same keys
	size_t clear_above = 16384;                   // a cache beyond this many entries is dropped (with its memo) when the next pass is listed
	bool use_memo = true;
	std::vector<pcrhost::Seed> tmp; std::vector<pcrhost::FoldSeed> tmp3;
	// the first sweep's record of a seeded orientation, and per group the end of its records and its chunk total
	struct Rec { const Entry *e; const uint32_t *run; uint32_t tag, pf_base; };
	std::vector<Rec> recs; std::vector<uint32_t> rec_end, g_total;
};

// The lists of a pass (what PlanLists of pcr_select.inc adds its other forms' lists to).
struct SeedLists {
	// second form of the seed scan: the seed list in groups of whole orientations, each within one launch's LDS budget; mask entries
	RawBuf<uint32_t> s2_seeds; RawBuf<Mask16> s2_masks;
	std::vector<uint32_t> s2_group_end, s2_group_offmask, s2_group_or, s2_group_nor;   // per group: end in the seed list, forward-seed slot offsets, first orientation, orientations spanned
	RawBuf<uint32_t> s3_prefix;                    // third form: the pass's chunk list
	RawBuf<uint8_t> s3_spans;                      // third form: per seed of s2_seeds the next bases it reads, lo | hi << 2
};

inline Entry *derive(Lister &Z, Cache &C, const Key &key, const Planes &m, bool third, bool fold)
{
	Entry e;
	Z.tmp.clear();
	if(third){
		Z.tmp3.clear();
		e.seedable = pcrhost::orientation_index_seeds(m, key.floor_, fold, Z.tmp3, Z.tmp);
		e.alloc((uint32_t)Z.tmp3.size(), true);
		uint8_t *sp = (uint8_t *)e.spans();
		for(size_t k = 0;k < Z.tmp3.size();++k){
			const pcrhost::FoldSeed &sd = Z.tmp3[k];
			e.block[k] = (sd.code << 14) | ((uint32_t)sd.off << 9); sp[k] = (uint8_t)(sd.lo | (sd.hi << 2)); e.off_mask |= 1u << sd.off;
		}
	}
	else{
		e.seedable = pcrhost::orientation_seeds(m, key.floor_, 0, Z.tmp, nullptr, 9);
		e.alloc((uint32_t)Z.tmp.size(), false);
		for(size_t k = 0;k < Z.tmp.size();++k){ const pcrhost::Seed &sd = Z.tmp[k]; e.block[k] = (sd.code << 14) | ((uint32_t)sd.off << 9); e.off_mask |= 1u << sd.off; }
	}
	e.mask = mask_of(m);
	return &C.map.emplace(key, std::move(e)).first->second;
}

// The exclusive running chunk counts of the entry's seeds in the set: the slot of the set's generation, made on a miss in the
// slot that is next in turn.
inline int chunk_slot(Entry &e, const SetIndex &S)
{
	for(int s = 0;s < CHUNK_SETS;++s){ if(e.gen[s] == S.generation) return s; }
	const int s = (int)e.next_slot; e.next_slot = (e.next_slot + 1u) % CHUNK_SETS;
	const uint32_t *const sd = e.seeds(); const uint8_t *const sp = e.spans(); uint32_t *const out = e.run(s);
	uint32_t run = 0;
	for(uint32_t k = 0;k < e.n;++k){
		const uint32_t key4 = (sd[k] >> 14) << 2, span = sp[k];
		out[k] = run; run += (S.start[key4 + (span >> 2) + 1u] - S.start[key4 + (span & 3u)] + 63u) >> 6;
	}
	e.total[s] = run; e.gen[s] = S.generation;
	return s;
}

// The seeds of a pass: per orientation from the cache (derived on a miss), listed as code << 14 | slot offset << 9 | orientation
// WITHIN ITS GROUP, in groups of whole orientations that each fit one launch (lim).  S3 (optional): the set whose position index
// the third form will read; the seeds are then the third cache's (fold: the oligo's folded seeds where they read less), a span byte
// per seed goes beside them (s3_spans), and the chunk list of every group (s3_prefix: the running number of 64-entry chunks of the
// group's seeds' spans, its total behind it) is made alongside.  Without S3 both of those lists come back empty.
// or_seed / or_plain receive the orientations with and without a seed structure, irr_off_mask the slot offsets at which forward
// seeds sit.  false: an orientation whose seeds alone exceed one launch, or too many groups -- the lists are then unspecified.
inline bool list_seeds(Lister &Z, const Limits &lim, const pcrhost::Candidate *cand, size_t n_cand, const SetIndex *S3, bool fold,
	SeedLists &L, std::vector<uint32_t> &or_seed, std::vector<uint32_t> &or_plain, uint32_t &irr_off_mask)
{
	const uint32_t n_or = 2*(uint32_t)n_cand;
	const bool third = S3 != nullptr;
	L.s2_seeds.clear(); L.s3_prefix.clear(); L.s3_spans.clear();
	L.s2_group_end.clear(); L.s2_group_offmask.clear(); L.s2_group_or.clear(); L.s2_group_nor.clear();
	irr_off_mask = 0;
	L.s2_masks.resize(n_or);
	if(Z.second.map.size() > Z.clear_above) Z.second.clear();
	if(Z.third.map.size() > Z.clear_above) Z.third.clear();
	Cache &C = third ? Z.third : Z.second;
	if(Z.use_memo && C.memo.size() < n_or) C.memo.resize(n_or, Cache::Slot{Key{0, 0, 0, 0, 0}, nullptr});
	auto fits = [&lim](size_t n, uint32_t g_or){ return g_or <= lim.max_or && n <= lim.max_seeds && lim.lds_fixed + 17*(size_t)g_or + 8*n <= lim.lds_budget; };
	Z.recs.clear(); Z.rec_end.clear(); Z.g_total.clear();
	// first sweep: every orientation's entry, the groups, the totals
	size_t n_out = 0, group_begin = 0; uint32_t group_mask = 0, group_or0 = 0, group_last = 0, pf_run = 0;
	Mask16 *const masks = L.s2_masks.data();
	for(uint32_t o = 0;o < n_or;++o){
		const pcrhost::Candidate &c = cand[o >> 1];
		const Planes &m = (o & 1u) ? c.rc : c.fwd;
		const Key key = {m.a, m.c, m.g, m.t, c.floor_};
		Entry *e;
		Cache::Slot *const memo = Z.use_memo ? &C.memo[o] : nullptr;
		if(memo && memo->e && memo->key == key) e = memo->e;
		else{
			auto it = C.map.find(key);
			e = it != C.map.end() ? &it->second : derive(Z, C, key, m, third, fold);
			if(memo){ memo->key = key; memo->e = e; }
		}
		masks[o] = e->mask;
		if(!e->seedable){ or_plain.push_back(o); continue; }
		or_seed.push_back(o);
		// the group spans orientations [group_or0, o]: unseedable ones in between only take an (unused) id
		if(!fits(n_out - group_begin + e->n, o - group_or0 + 1)){              // close the group, open the next at this orientation
			if(!fits(e->n, 1) || L.s2_group_end.size() + 1 >= lim.max_groups) return false;
			L.s2_group_end.push_back((uint32_t)n_out); L.s2_group_offmask.push_back(group_mask); L.s2_group_or.push_back(group_or0); L.s2_group_nor.push_back(group_last - group_or0 + 1);
			Z.rec_end.push_back((uint32_t)Z.recs.size()); Z.g_total.push_back(pf_run);
			group_begin = n_out; group_mask = 0; group_or0 = o; pf_run = 0;      // (the chunk list of the next group starts at 0)
		}
		group_last = o;
		Lister::Rec r = { e, nullptr, o - group_or0, pf_run };
		if(third){ const int s = chunk_slot(*e, *S3); r.run = e->run(s); pf_run += e->total[s]; }
		Z.recs.push_back(r);
		n_out += e->n;
		if(!(o & 1u)){ irr_off_mask |= e->off_mask; group_mask |= e->off_mask; }   // slot offsets at which forward seeds sit (irregular-word scan)
	}
	L.s2_group_end.push_back((uint32_t)n_out); L.s2_group_offmask.push_back(group_mask); L.s2_group_or.push_back(group_or0);
	L.s2_group_nor.push_back(or_seed.empty() ? 0u : group_last - group_or0 + 1);
	Z.rec_end.push_back((uint32_t)Z.recs.size()); Z.g_total.push_back(pf_run);
	// the lists, sized once
	L.s2_seeds.resize(n_out);
	if(third){ L.s3_spans.resize(n_out); L.s3_prefix.resize(n_out + Z.rec_end.size()); }
	// second sweep
	uint32_t *__restrict out = L.s2_seeds.data(), *__restrict pf = L.s3_prefix.data(); uint8_t *__restrict spans = L.s3_spans.data();
	size_t r0 = 0;
	for(size_t g = 0;g < Z.rec_end.size();++g){
		for(size_t i = r0;i < Z.rec_end[g];++i){
			const Lister::Rec &r = Z.recs[i];
			const uint32_t n = r.e->n, tag = r.tag;
			const uint32_t *__restrict sd = r.e->seeds();
			for(uint32_t k = 0;k < n;++k) out[k] = sd[k] | tag;
			out += n;
			if(third){
				const uint32_t *__restrict run = r.run; const uint32_t base = r.pf_base;
				for(uint32_t k = 0;k < n;++k) pf[k] = base + run[k];
				pf += n;
				if(n){ memcpy(spans, r.e->spans(), n); spans += n; }
			}
		}
		r0 = Z.rec_end[g];
		if(third) *pf++ = Z.g_total[g];                                     // the group's total
	}
	return true;
}

// Third form: the chunks of every launch group dealt to G workgroups in equal contiguous shares, and per workgroup the first seed of
// its share (a merge walk over the group's chunk list).  Launch: { struct { uint32_t start[max_wg + 1]; } W; uint32_t n_chunks,
// per_wg, slice_cap, n_irr_wg; }.  G_all: the launch's workgroups; seeds_per_turn: the seeds a workgroup of the irregular words
// looks up per turn.  false: some group's largest slice does not fit lds_budget (many seeds whose runs are empty side by side).
template<class Launch>
inline bool plan_slices(const SeedLists &PL, std::vector<Launch> &launch, uint32_t G_all, uint32_t seeds_per_turn, uint32_t max_wg, size_t lds_budget, bool with_irr)
{
	launch.resize(PL.s2_group_end.size());
	size_t g_begin = 0, g_prefix = 0;
	for(size_t g = 0;g < PL.s2_group_end.size();++g){
		const uint32_t ns = PL.s2_group_end[g] - (uint32_t)g_begin;
		g_begin = PL.s2_group_end[g];
		const uint32_t *P = PL.s3_prefix.data() + g_prefix;                  // the group's chunk list, [ns + 1]
		g_prefix += (size_t)ns + 1;
		Launch &L = launch[g];
		// the launch's first workgroups look the irregular words up (16 seeds per wave turn) and leave the chunks to the others: the two
		// chains of dependent loads then run side by side; at most a quarter of the launch
		L.n_irr_wg = with_irr ? std::min<uint32_t>((ns + seeds_per_turn - 1u)/seeds_per_turn, G_all/4u) : 0u;
		const uint32_t G = (G_all - L.n_irr_wg) & ~1u;                       // even: a paired launch gives two neighbours' shares to one workgroup (pair_slices)
		L.n_chunks = P[ns]; L.per_wg = std::max<uint32_t>(1u, (L.n_chunks + G - 1u)/G); L.slice_cap = 2;
		if(ns == 0) continue;
		uint32_t at = 0;
		for(uint32_t w = 0;w <= G;++w){
			const uint64_t target = (uint64_t)w*L.per_wg;
			while(at + 1u < ns && P[at + 1u] <= target) ++at;
			L.W.start[w] = at;
		}
		for(uint32_t w = G + 1;w <= max_wg;++w) L.W.start[w] = at;
		for(uint32_t w = 0;w < G;++w) L.slice_cap = std::max(L.slice_cap, std::min(L.W.start[w + 1] + 2u, ns + 1u) - L.W.start[w]);
		if(17*(size_t)PL.s2_group_nor[g] + 9*(size_t)L.slice_cap + 64 > lds_budget) return false;   // masks, floors | slice of the chunk list, the seeds and their spans
	}
	return true;
}

} // namespace pcrseed

#endif
