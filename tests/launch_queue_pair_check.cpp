// Stand-alone check of the PAIRS of pcramp_amd/csrc/pcr_launch_queue.hpp (no GPU, no HIP): built with a sanitizer and run by
// test_launch_queue_pair_host.py.  Jobs are small records; the launcher thread appends what it runs, alone or as a pair, to a log.
#include "../pcramp_amd/csrc/pcr_launch_queue.hpp"

#include <stdio.h>
#include <stdlib.h>
#include <vector>

#define CHECK(cond) do{ if(!(cond)){ fprintf(stderr, "launch_queue_pair_check: %s:%d: %s\n", __FILE__, __LINE__, #cond); exit(1); } }while(0)

struct Job { int id; int owner; bool holdable; bool fail; };
struct Ran { int a, b; };                             // b < 0: a ran alone

int main()
{
	std::vector<Ran> log; std::mutex log_m;
	std::atomic<bool> may_hold{true};
	auto make = [&](unsigned cap_us){
		auto *q = new pcrq::LaunchQueue(
			[&](void *j, std::string &err) -> int { Job *J = (Job *)j; { std::lock_guard<std::mutex> lk(log_m); log.push_back(Ran{J->id, -1}); } if(J->fail){ err = "alone"; return 7; } return 0; },
			[](void *){}, nullptr, 50);
		pcrq::LaunchQueue::Pairing p;
		p.holdable = [](void *j){ return ((Job *)j)->holdable; };
		p.may_hold = [&](void *){ return may_hold.load(); };
		p.can_pair = [](void *a, void *b){ return ((Job *)a)->owner != ((Job *)b)->owner && ((Job *)b)->holdable; };
		p.run_pair = [&](void *a, void *b, std::string &err) -> int {
			Job *A = (Job *)a, *B = (Job *)b;
			{ std::lock_guard<std::mutex> lk(log_m); log.push_back(Ran{A->id, B->id}); }
			if(A->fail || B->fail){ err = "pair"; return 9; }
			return 0;
		};
		p.cap_us = cap_us;
		q->set_pairing(std::move(p));
		return q;
	};
	auto take = [&]{ std::lock_guard<std::mutex> lk(log_m); std::vector<Ran> l; l.swap(log); return l; };
	{
		// A B C A B C A from three owners: (0,1) (2,3) (4,5) pair, 6 is held until its owner's flush releases it
		pcrq::LaunchQueue *q = make(10u*1000u*1000u);
		pcrq::Client c[3]; Job j[7];
		for(int i = 0;i < 7;++i){ j[i] = Job{i, i % 3, true, false}; q->push(&c[i % 3], &j[i], (uint32_t)i); }
		while(c[1].queued.load() || c[2].queued.load()) pcrq::cpu_relax();   // (no flush: a flush by anybody releases a held job)
		const auto t_end = std::chrono::steady_clock::now() + std::chrono::milliseconds(2);
		while(std::chrono::steady_clock::now() < t_end) pcrq::cpu_relax();
		CHECK(c[0].queued.load() == 1);                 // (the seventh job: held, nobody has asked for it)
		q->flush(&c[0]);
		std::vector<Ran> l = take();
		CHECK(l.size() == 4 && l[0].a == 0 && l[0].b == 1 && l[1].a == 2 && l[1].b == 3 && l[2].a == 4 && l[2].b == 5 && l[3].a == 6 && l[3].b == -1);
		// a successor that cannot pair (same owner; not holdable): the held job runs alone FIRST
		Job s[4] = { {10, 0, true, false}, {11, 0, true, false}, {12, 1, false, false}, {13, 2, true, false} };
		pcrq::Client *own[4] = { &c[0], &c[0], &c[1], &c[2] };
		for(int i = 0;i < 4;++i) q->push(own[i], &s[i], 0);
		q->wait_empty();
		l = take();
		CHECK(l.size() == 4);
		for(int i = 0;i < 4;++i) CHECK(l[i].a == 10 + i && l[i].b == -1);
		// a failed pair poisons both clients; their later jobs are dropped, the third client's still run
		Job f[5] = { {20, 0, true, true}, {21, 1, true, false}, {22, 0, true, false}, {23, 1, true, false}, {24, 2, false, false} };
		pcrq::Client *fo[5] = { &c[0], &c[1], &c[0], &c[1], &c[2] };
		for(int i = 0;i < 5;++i) q->push(fo[i], &f[i], 100u + (uint32_t)i);
		q->wait_empty();
		l = take();
		CHECK(l.size() == 2 && l[0].a == 20 && l[0].b == 21 && l[1].a == 24 && l[1].b == -1);
		int code; std::string msg; uint32_t tag;
		CHECK(c[0].take_error(code, msg, tag) && code == 9 && msg == "pair" && tag == 100);
		CHECK(c[1].take_error(code, msg, tag) && code == 9 && tag == 101);
		CHECK(!c[2].take_error(code, msg, tag));
		q->stop(); delete q;
	}
	{
		// the owner's rule ends the hold (may_hold false), and so does the time cap: a lone job always runs
		pcrq::LaunchQueue *q = make(2000);
		pcrq::Client c; Job a{30, 0, true, false}, b{31, 0, true, false};
		may_hold.store(false);
		q->push(&c, &a, 0);
		while(c.queued.load()) pcrq::cpu_relax();
		may_hold.store(true);
		q->push(&c, &b, 0);                             // nobody flushes: the 2 ms cap releases it
		while(c.queued.load()) pcrq::cpu_relax();
		std::vector<Ran> l = take();
		CHECK(l.size() == 2 && l[0].a == 30 && l[1].a == 31 && l[1].b == -1);
		q->stop(); delete q;
	}
	{
		// stop() with a job held: the thread is joined, the job is dropped or run, nothing hangs
		pcrq::LaunchQueue *q = make(10u*1000u*1000u);
		pcrq::Client c; Job a{40, 0, true, false};
		q->push(&c, &a, 0);
		q->stop();
		CHECK(c.queued.load() == 0);
		delete q;
	}
	printf("launch queue pairs ok\n");
	return 0;
}
