// The folded seeds of the position-index scan (pcrhost::orientation_fold_seeds, pcramp_amd/csrc/pcr_host.hpp) on the CPU, as a
// stand-alone program: tests/test_seed_fold_host.py compiles it with -fsanitize=address,undefined and runs it.
//
// The filter must be sound: a 32-base window that matches an oligo in at least `floor` of its occupied slots must be found by
// SOME folded seed -- its bases off .. off + 8 spell the seed's code and base off + 9 lies in lo..hi.  Checked for every length
// 18 ... 25, floors unsigned(size * t) for t in {0.81, 0.9, 1.0}, every centring a 32-slot word allows and EVERY set of at most
// k = size - floor mismatching slots (replacement bases and the bases around the oligo random, fixed seed); the same for oligos
// with one IUPAC slot at every position in turn (so also at the tenth position of every block) and with 2-3 random ones, at
// the first and the last centring and every second or third one between.
// For plain oligos at 0.9 the entries read are the figures the layout search was chosen for, never more than the plain 9-gram
// list reads, and no folded seed sits at an offset above 22 (base off + 9 must lie inside the window).  The list the planner
// takes (orientation_index_seeds: the fold, or the plain list with span A..T where no fold exists or it reads no less) gets the
// same exhaustive check.
#include <stdio.h>
#include <stdlib.h>
#include <unordered_map>
#include "../pcramp_amd/csrc/pcr_host.hpp"

using pcrhost::Planes;
using pcrhost::FoldSeed;

static uint64_t g_rng = 0x243F6A8885A308D3ull;
static uint32_t rnd(uint32_t n) { g_rng = g_rng*6364136223846793005ull + 1442695040888963407ull; return (uint32_t)((g_rng >> 33) % n); }
static unsigned long long g_windows = 0, g_cases = 0, g_unseedable = 0;
static int g_fail = 0;

#define CHECK(c, ...) do{ if(!(c)){ printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); if(++g_fail > 20) exit(1); } }while(0)

static Planes planes_of_sets(const unsigned *sets /* [32], 4-bit base sets, 0 = empty slot */)
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

struct Index {                                       // the folded seeds of one orientation by (offset, code)
	std::vector<int> offs;
	std::unordered_map<uint32_t, std::vector<FoldSeed> > by_key;
	void build(const std::vector<FoldSeed> &seeds)
	{
		offs.clear(); by_key.clear();
		for(const FoldSeed &f : seeds){
			if(std::find(offs.begin(), offs.end(), (int)f.off) == offs.end()) offs.push_back(f.off);
			by_key[((uint32_t)f.off << 18) | f.code].push_back(f);
		}
	}
	bool finds(const uint8_t *win) const
	{
		for(int off : offs){
			uint32_t code = 0;
			for(int j = 0;j < 9;++j) code |= (uint32_t)win[off + j] << (2*j);
			auto it = by_key.find(((uint32_t)off << 18) | code);
			if(it == by_key.end()) continue;
			for(const FoldSeed &f : it->second){
				if(f.lo == 0 && f.hi == 3) return true;                       // no constraint: base off + 9 is not looked at (it may lie behind the window)
				if(win[off + 9] >= f.lo && win[off + 9] <= f.hi) return true;
			}
		}
		return false;
	}
};

// every set of at most k mismatching slots among the occupied ones: the window holds a base of the slot's set where it matches, a base
// outside it where it does not (slots whose set is N cannot mismatch and are left out), random bases around the oligo
static void all_mismatch_sets(const unsigned *sets, int first, int size, int k, const Index &ix, const char *what)
{
	std::vector<int> can;
	for(int j = first;j < first + size;++j){ if(sets[j] != 15u) can.push_back(j); }
	std::vector<int> pick;
	uint8_t win[32];
	auto pick_base = [](unsigned set){ unsigned b; do b = rnd(4); while(!(set & (1u << b))); return (uint8_t)b; };
	// (iterative enumeration of the subsets of `can` with at most k members, in lexicographic order)
	for(;;){
		for(int j = 0;j < 32;++j) win[j] = (j >= first && j < first + size) ? pick_base(sets[j]) : (uint8_t)rnd(4);
		for(int j : pick) win[can[j]] = pick_base(~sets[can[j]] & 15u);
		++g_windows;
		if(!ix.finds(win)){
			printf("FAIL %s: first %d size %d k %d, mismatching slots", what, first, size, k);
			for(int j : pick) printf(" %d", can[j]);
			printf(": no folded seed matches\n");
			if(++g_fail > 20) exit(1);
		}
		// next subset
		if((int)pick.size() < k && (pick.empty() ? !can.empty() : pick.back() + 1 < (int)can.size())){ pick.push_back(pick.empty() ? 0 : pick.back() + 1); continue; }
		while(!pick.empty() && pick.back() + 1 >= (int)can.size()) pick.pop_back();
		if(pick.empty()) break;
		++pick.back();
	}
}

struct CaseOut { bool folds; unsigned cost4, n_seeds, n_plain; };

static void check_list(const std::vector<FoldSeed> &seeds, unsigned cost4, bool every_offset, const char *what, int first, int size, float t)
{
	unsigned sum = 0;
	for(const FoldSeed &f : seeds){
		CHECK(f.code < (1u << 18) && f.lo <= f.hi && f.hi <= 3, "%s: malformed seed", what);
		// (a seed that constrains base off + 9 needs it inside the window; the fold's own lists keep every offset there)
		if(every_offset || f.lo != 0 || f.hi != 3) CHECK(f.off <= 22, "%s: offset %u (first %d size %d t %.2f)", what, (unsigned)f.off, first, size, (double)t);
		CHECK(f.off <= 23, "%s: offset %u", what, (unsigned)f.off);
		sum += (unsigned)(f.hi - f.lo + 1);
	}
	CHECK(sum == cost4, "%s: cost %u reported, %u listed", what, cost4, sum);
	for(size_t i = 0;i < seeds.size();++i){
		for(size_t j = i + 1;j < seeds.size();++j) CHECK(seeds[i].off != seeds[j].off || seeds[i].code != seeds[j].code, "%s: a (offset, code) listed twice", what);
	}
}

// the fold itself (orientation_fold_seeds), and the list the planner takes (orientation_index_seeds: the fold, or the plain 9-gram list
// with span A..T where there is no fold or it reads no less)
static CaseOut run_case(const unsigned *sets, int first, int size, float t, const char *what)
{
	const Planes m = planes_of_sets(sets);
	const uint32_t floor_ = (unsigned)((float)size*t);
	const int k = size - (int)floor_;
	std::vector<FoldSeed> seeds, taken; std::vector<pcrhost::Seed> tmp, plain;
	unsigned cost4 = 0, taken4 = 0;
	CaseOut out = {false, 0, 0, 0};
	++g_cases;
	const bool plain_ok = pcrhost::orientation_seeds(m, floor_, 0, plain, nullptr, 9);
	out.folds = pcrhost::orientation_fold_seeds(m, floor_, seeds, tmp, &cost4);
	out.n_plain = (unsigned)plain.size();
	Index ix;
	if(!out.folds){ ++g_unseedable; CHECK(seeds.empty(), "%s: seeds without a structure", what); }
	else{
		check_list(seeds, cost4, true, what, first, size, t);
		ix.build(seeds);
		all_mismatch_sets(sets, first, size, k, ix, what);
		out.cost4 = cost4; out.n_seeds = (unsigned)seeds.size();
	}
	const bool taken_ok = pcrhost::orientation_index_seeds(m, floor_, true, taken, tmp, &taken4);
	CHECK(taken_ok == plain_ok, "%s: the scan's list exists exactly where the 9-gram list does (first %d size %d)", what, first, size);
	if(taken_ok){
		check_list(taken, taken4, false, what, first, size, t);
		CHECK(taken4 <= 4u*(unsigned)plain.size(), "%s: the scan reads more (%u quarter runs) than the %zu plain seeds", what, taken4, plain.size());
		if(out.folds && plain_ok) CHECK(taken4 == std::min(cost4, 4u*(unsigned)plain.size()), "%s: not the cheaper list", what);
		if(!out.folds || taken4 != cost4){ ix.build(taken); all_mismatch_sets(sets, first, size, k, ix, what); }
	}
	else CHECK(taken.empty(), "%s: seeds of an unseedable orientation", what);
	return out;
}

int main()
{
	// quarter runs read / folded seeds of a plain oligo at select threshold 0.9 (18: 11.75 runs ... 21-25: 15.5 runs)
	static const unsigned want_cost4[26] = {0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0, 47, 35, 32, 62, 62, 62, 62, 62};
	static const unsigned want_seeds[26] = {0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0, 32, 29, 29, 56, 56, 56, 56, 56};
	static const float thr[3] = {0.81f, 0.9f, 1.0f};
	unsigned sets[32];
	for(int size = 18;size <= 25;++size){
		for(int ti = 0;ti < 3;++ti){
			for(int first = 0;first + size <= 32;++first){
				for(int j = 0;j < 32;++j) sets[j] = (j >= first && j < first + size) ? 1u << rnd(4) : 0u;
				const CaseOut r = run_case(sets, first, size, thr[ti], "plain oligo");
				if(ti == 1){
					CHECK(r.folds, "plain %d-mer at 0.9 has no fold", size);
					CHECK(r.cost4 == want_cost4[size], "plain %d-mer at 0.9 (first %d): %u quarter runs, expected %u", size, first, r.cost4, want_cost4[size]);
					CHECK(r.n_seeds == want_seeds[size], "plain %d-mer at 0.9 (first %d): %u folded seeds, expected %u", size, first, r.n_seeds, want_seeds[size]);
					CHECK(r.cost4 <= 4u*r.n_plain && r.cost4 < 4u*r.n_plain, "plain %d-mer at 0.9: no fewer entries than the plain list", size);
				}
			}
		}
	}
	const unsigned long long plain_windows = g_windows;
	// IUPAC slots (two- and three-fold sets that hold a random base of their own), select threshold 0.9 and 0.81
	static const unsigned two[6] = {3, 5, 9, 6, 10, 12}, three[4] = {7, 11, 13, 14};
	for(int size = 18;size <= 25;++size){
		for(int first = 0;first + size <= 32;first += (size & 1) ? 3 : 2){          // (a sample of the centrings: the ends and every second or third between)
			for(int at = 0;at < size;++at){                                          // one slot, at every position: also the tenth of every block
				for(int j = 0;j < 32;++j) sets[j] = (j >= first && j < first + size) ? 1u << rnd(4) : 0u;
				sets[first + at] = two[rnd(6)];
				run_case(sets, first, size, 0.9f, "one IUPAC slot");
			}
			for(int rep = 0;rep < 6;++rep){                                          // two or three slots anywhere
				for(int j = 0;j < 32;++j) sets[j] = (j >= first && j < first + size) ? 1u << rnd(4) : 0u;
				const int n = 2 + (rep & 1);
				for(int i = 0;i < n;++i) sets[first + (int)rnd((uint32_t)size)] = (rnd(3) == 0) ? three[rnd(4)] : two[rnd(6)];
				run_case(sets, first, size, (rep < 4) ? 0.9f : 0.81f, "2-3 IUPAC slots");
			}
		}
		{                                                                            // ... and at the last centring
			const int first = 32 - size;
			for(int at = 0;at < size;++at){
				for(int j = 0;j < 32;++j) sets[j] = (j >= first && j < first + size) ? 1u << rnd(4) : 0u;
				sets[first + at] = two[rnd(6)];
				run_case(sets, first, size, 0.9f, "one IUPAC slot, last centring");
			}
		}
	}
	printf("%llu cases (%llu without a 10-gram structure), %llu windows (%llu of plain oligos)\n", g_cases, g_unseedable, g_windows, plain_windows);
	if(g_fail){ printf("%d failures\n", g_fail); return 1; }
	printf("seed fold ok\n");
	return 0;
}
