// Stand-alone check of pcramp_amd/csrc/pcr_launch_queue.hpp (no GPU, no HIP): built with a sanitizer and run by
// test_launch_queue_host.py.  Two producer "handles" push jobs that append to a vector; the launcher thread serves them.
// Exit status 0 and a last line "launch queue ok" when every check holds.
#include "../pcramp_amd/csrc/pcr_launch_queue.hpp"

#include <stdio.h>
#include <stdlib.h>
#include <vector>

#define CHECK(cond) do{ if(!(cond)){ fprintf(stderr, "launch_queue_check: %s:%d: %s\n", __FILE__, __LINE__, #cond); exit(1); } }while(0)

struct Job { int handle, serial; bool fail, slow; };

// threads of this process, from the kernel's own count
static int n_threads()
{
	FILE *f = fopen("/proc/self/status", "r");
	if(!f) return -1;
	char line[256]; int n = -1;
	while(fgets(line, sizeof(line), f)){ if(sscanf(line, "Threads: %d", &n) == 1) break; }
	fclose(f);
	return n;
}

int main()
{
	{ std::thread warm([]{}); warm.join(); }      // (a sanitizer starts its own helper thread with the first thread of the program: before the count)
	const int threads_before = n_threads();
	std::vector<int> log;                  // handle*1000 + serial of every job RUN, in the order run (launcher thread; read after a flush)
	std::vector<int> dropped;              // ... of every job handed back without having run
	std::vector<int> ran_flag(4000, 0);
	std::atomic<int> started{0};
	{
		pcrq::LaunchQueue q(
			[&](void *p, std::string &err) -> int {
				Job *j = (Job *)p;
				if(j->slow) std::this_thread::sleep_for(std::chrono::milliseconds(2));
				log.push_back(j->handle*1000 + j->serial);
				ran_flag[j->handle*1000 + j->serial] = 1;
				if(j->fail){ err = "job failed on purpose"; return -7; }
				return 0;
			},
			[&](void *p){ Job *j = (Job *)p; if(!ran_flag[j->handle*1000 + j->serial]) dropped.push_back(j->handle*1000 + j->serial); delete j; },
			[&]{ started.fetch_add(1); },
			50);
		CHECK(!q.thread_alive());                                         // lazily: no thread before the first push
		pcrq::Client A, B;

		// 1. FIFO across producers: one thread pushes for both handles alternately, as a caller with several handles on one stream does
		std::vector<int> want;
		for(int i = 0;i < 200;++i){
			pcrq::Client &c = (i % 3 == 0) ? B : A; const int h = (i % 3 == 0) ? 2 : 1;
			q.push(&c, new Job{h, i, false, i < 4}, (uint32_t)i);
			want.push_back(h*1000 + i);
		}
		// 2. flush returns only when the handle's own jobs are done (the last job pushed is A's: everything before it ran too)
		q.flush(&A);
		CHECK(A.queued.load() == 0);
		size_t nA = 0; for(int v : log){ if(v/1000 == 1) ++nA; }
		CHECK(nA == 133);
		q.flush(&B);
		CHECK(log == want);
		CHECK(started.load() == 1 && q.thread_alive());
		CHECK(A.max_depth >= 2);                                          // (the first jobs are slow: the queue fills behind them)
		CHECK(A.n_pushed == 133 && B.n_pushed == 67);

		// 3. two producer THREADS, each with its own handle: per-handle order is kept, and flush waits for the handle's jobs
		log.clear();
		auto producer = [&](pcrq::Client *c, int h){
			for(int i = 0;i < 300;++i){
				q.push(c, new Job{h, i, false, false}, (uint32_t)i);
				if(i % 50 == 49){ q.flush(c); CHECK(c->queued.load() == 0); }
			}
		};
		{
			std::thread t1(producer, &A, 1), t2(producer, &B, 2);
			t1.join(); t2.join();
		}
		q.wait_empty();
		CHECK(log.size() == 600);
		int next[3] = {0, 0, 0};
		for(int v : log){ CHECK(v%1000 == next[v/1000]); ++next[v/1000]; }

		// 4. a failed job poisons its handle: its later jobs are dropped, the other handle's jobs still run
		log.clear(); dropped.clear();
		std::fill(ran_flag.begin(), ran_flag.end(), 0);
		q.push(&A, new Job{1, 0, false, true}, 100);
		q.push(&A, new Job{1, 1, true, false}, 101);                      // fails
		q.push(&B, new Job{2, 0, false, false}, 200);
		q.push(&A, new Job{1, 2, false, false}, 102);                     // dropped
		q.push(&B, new Job{2, 1, false, false}, 201);
		q.push(&A, new Job{1, 3, false, false}, 103);                     // dropped
		q.flush(&A); q.flush(&B);
		CHECK((log == std::vector<int>{1000, 1001, 2000, 2001}));
		CHECK((dropped == std::vector<int>{1002, 1003}));
		int code = 0; std::string msg; uint32_t tag = 0;
		CHECK(!B.take_error(code, msg, tag));
		CHECK(A.take_error(code, msg, tag) && code == -7 && tag == 101 && msg == "job failed on purpose");
		CHECK(!A.take_error(code, msg, tag));                             // reported once; the handle takes jobs again
		q.push(&A, new Job{1, 4, false, false}, 104);
		q.flush(&A);
		CHECK(log.back() == 1004);

		// 5. stop and join: jobs still queued are handed back, no thread is left
		log.clear(); dropped.clear();
		std::fill(ran_flag.begin(), ran_flag.end(), 0);
		q.push(&A, new Job{1, 0, false, true}, 0);
		for(int i = 1;i < 20;++i) q.push(&B, new Job{2, i, false, true}, (uint32_t)i);
		q.stop();
		CHECK(!q.thread_alive());
		CHECK(log.size() + dropped.size() == 20);
		CHECK(A.queued.load() == 0 && B.queued.load() == 0);
	}
	const int threads_after = n_threads();
	CHECK(threads_before < 0 || threads_after == threads_before);          // nothing but the main thread (and the sanitizer's own, as before)
	// a queue that was never used starts and leaves no thread
	{
		pcrq::LaunchQueue idle([](void *, std::string &){ return 0; }, [](void *){}, nullptr, 50);
		CHECK(!idle.thread_alive());
	}
	CHECK(n_threads() == threads_after);
	printf("launch queue ok\n");
	return 0;
}
