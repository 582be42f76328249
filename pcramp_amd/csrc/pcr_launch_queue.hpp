// An ordered launcher: a FIFO of jobs served by ONE thread, shared by several producers ("clients": the library's handles on one
// stream).  The thread is created by the first push and joined by stop(); between jobs it spins on the queue for a bounded time and
// then blocks on a condition variable.  No HIP here: the jobs are opaque, the owner passes what runs them (tested on the CPU,
// tests/launch_queue_check.cpp).
//
// PAIRS (optional: set_pairing, before the first push).  A job the owner calls holdable is not run at once: the thread keeps it
// while the owner says holding costs nothing (may_hold) and looks for the job behind it.  If that one can pair with it (can_pair)
// the two are run by ONE call (run_pair); a failure poisons both clients.  Otherwise the held job runs alone, first: jobs run in
// the order they were pushed, whatever pairs.  The hold ends -- and the job runs alone -- as soon as anybody calls flush() or
// stop(), or after cap_us.
//
// Who may call what: push(), flush() and the client's fields marked (owner) belong to the thread that uses the client's handle
// (one at a time, as the handle itself); run/done are called by the launcher thread only; stop() by whoever owns the queue,
// after the last client has flushed.
#ifndef PCR_LAUNCH_QUEUE_HPP
#define PCR_LAUNCH_QUEUE_HPP

#include <stdint.h>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <functional>
#include <mutex>
#include <string>
#include <thread>

namespace pcrq {

inline void cpu_relax()
{
#if defined(__x86_64__) || defined(__i386__)
	__builtin_ia32_pause();
#else
	std::this_thread::yield();
#endif
}

// One per producer.  A failed job POISONS its client: the client's later jobs are dropped, not run, until the owner has taken
// the error (take_error).
struct Client {
	std::atomic<uint32_t> queued{0};        // jobs pushed and neither run nor dropped yet
	std::atomic<bool> poisoned{false};
	// written by the launcher thread before `poisoned` is set (release), read by the owner after it has seen it (acquire)
	int err_code = 0; std::string err_msg; uint32_t err_tag = 0;
	uint64_t n_pushed = 0; uint32_t max_depth = 0;   // (owner) jobs pushed; the most of this client's jobs in the queue at once
	// (owner) the error of the job that poisoned the client, once; the client takes jobs again afterwards.  Call after flush().
	bool take_error(int &code, std::string &msg, uint32_t &tag)
	{
		if(!poisoned.load(std::memory_order_acquire)) return false;
		code = err_code; msg = err_msg; tag = err_tag;
		poisoned.store(false, std::memory_order_release);
		return true;
	}
};

class LaunchQueue {
public:
	typedef std::function<int(void *job, std::string &err)> RunFn;   // 0: done; anything else poisons the job's client
	typedef std::function<void(void *job)> DoneFn;                   // the job was run or dropped: the queue is done with it
	LaunchQueue(RunFn run, DoneFn done, std::function<void()> on_start, unsigned spin_us)
		: run_(std::move(run)), done_(std::move(done)), on_start_(std::move(on_start)), spin_us_(spin_us) {}
	~LaunchQueue() { stop(); }
	struct Pairing {
		std::function<bool(void *job)> holdable;                 // could this job be one half of a pair at all?
		std::function<bool(void *job)> may_hold;                 // asked again and again while the job is held alone: false releases it
		std::function<bool(void *a, void *b)> can_pair;          // a was pushed before b
		std::function<int(void *a, void *b, std::string &err)> run_pair;   // 0: done; anything else poisons both clients
		unsigned cap_us = 0;                                     // the longest a job is held
	};
	void set_pairing(Pairing p) { pairing_ = std::move(p); has_pairing_ = true; }
	LaunchQueue(const LaunchQueue &) = delete;
	LaunchQueue &operator=(const LaunchQueue &) = delete;

	// tag: the owner's name for the job (comes back with its error)
	void push(Client *c, void *job, uint32_t tag)
	{
		const uint32_t depth = c->queued.fetch_add(1, std::memory_order_seq_cst) + 1;
		if(depth > c->max_depth) c->max_depth = depth;
		++c->n_pushed;
		bool wake;
		{
			std::lock_guard<std::mutex> lk(m_);
			if(!started_){ started_ = true; th_ = std::thread([this]{ work(); }); }
			q_.push_back(Item{c, job, tag});
			n_items_.store((uint32_t)q_.size(), std::memory_order_release);
			wake = worker_waiting_;
		}
		if(wake) cv_.notify_one();
	}
	// returns when every job of c pushed so far has been run or dropped
	void flush(Client *c)
	{
		if(c->queued.load(std::memory_order_seq_cst) == 0) return;
		flush_req_.fetch_add(1, std::memory_order_seq_cst);      // (a held job is released at once)
		const auto t_end = std::chrono::steady_clock::now() + std::chrono::microseconds(200);
		while(std::chrono::steady_clock::now() < t_end){
			if(c->queued.load(std::memory_order_seq_cst) == 0){ flush_req_.fetch_sub(1, std::memory_order_seq_cst); return; }
			cpu_relax();
		}
		flush_waiters_.fetch_add(1, std::memory_order_seq_cst);
		{
			std::unique_lock<std::mutex> lk(m_);
			cv_done_.wait(lk, [&]{ return c->queued.load(std::memory_order_seq_cst) == 0; });
		}
		flush_waiters_.fetch_sub(1, std::memory_order_seq_cst);
		flush_req_.fetch_sub(1, std::memory_order_seq_cst);
	}
	// returns when the queue holds no job and none is running
	void wait_empty()
	{
		flush_req_.fetch_add(1, std::memory_order_seq_cst);
		flush_waiters_.fetch_add(1, std::memory_order_seq_cst);
		{
			std::unique_lock<std::mutex> lk(m_);
			cv_done_.wait(lk, [&]{ return q_.empty() && !busy_; });
		}
		flush_waiters_.fetch_sub(1, std::memory_order_seq_cst);
		flush_req_.fetch_sub(1, std::memory_order_seq_cst);
	}
	// Jobs still queued are dropped; the thread is joined.  The queue does not start again.
	void stop()
	{
		{
			std::lock_guard<std::mutex> lk(m_);
			stop_ = true; stop_flag_.store(true, std::memory_order_release);
			if(!started_) started_ = true;          // (never started: no thread will be)
		}
		cv_.notify_all();
		if(th_.joinable()) th_.join();
	}
	bool thread_alive() const { return th_.joinable(); }

private:
	struct Item { Client *client; void *job; uint32_t tag; };

	bool pop(Item &it)
	{
		if(spin_us_){
			const auto t_end = std::chrono::steady_clock::now() + std::chrono::microseconds(spin_us_);
			while(n_items_.load(std::memory_order_acquire) == 0 && !stop_flag_.load(std::memory_order_acquire)){
				if(std::chrono::steady_clock::now() >= t_end) break;
				cpu_relax();
			}
		}
		std::unique_lock<std::mutex> lk(m_);
		worker_waiting_ = true;
		cv_.wait(lk, [&]{ return !q_.empty() || stop_; });
		worker_waiting_ = false;
		if(q_.empty()) return false;
		it = q_.front(); q_.pop_front();
		n_items_.store((uint32_t)q_.size(), std::memory_order_release);
		busy_ = true;
		return true;
	}
	static void poison(const Item &it, int rc, const std::string &err)
	{
		Client *const c = it.client;
		c->err_code = rc; c->err_msg = err; c->err_tag = it.tag;
		c->poisoned.store(true, std::memory_order_release);
	}
	bool runnable(const Item &it) const { return !stop_flag_.load(std::memory_order_acquire) && !it.client->poisoned.load(std::memory_order_acquire); }
	void retire(const Item &it)
	{
		done_(it.job);
		it.client->queued.fetch_sub(1, std::memory_order_seq_cst);
	}
	// `it` is held: wait for the job behind it.  true: `next` is that job, taken off the queue, and the two can pair.
	bool find_partner(const Item &it, Item &next)
	{
		const auto t_end = std::chrono::steady_clock::now() + std::chrono::microseconds(pairing_.cap_us);
		while(n_items_.load(std::memory_order_acquire) == 0){
			if(flush_req_.load(std::memory_order_seq_cst) || stop_flag_.load(std::memory_order_acquire)) return false;
			if(!pairing_.may_hold(it.job) || std::chrono::steady_clock::now() >= t_end) return false;
			cpu_relax();
		}
		std::lock_guard<std::mutex> lk(m_);
		if(q_.empty()) return false;
		const Item &front = q_.front();
		if(front.client->poisoned.load(std::memory_order_acquire) || !pairing_.can_pair(it.job, front.job)) return false;   // (it stays queued: the next turn takes it)
		next = front; q_.pop_front();
		n_items_.store((uint32_t)q_.size(), std::memory_order_release);
		return true;
	}
	void work()
	{
		if(on_start_) on_start_();
		Item it, next;
		while(pop(it)){
			bool paired = false;
			if(runnable(it)){
				std::string err;
				paired = has_pairing_ && pairing_.holdable(it.job) && find_partner(it, next);
				const int rc = paired ? pairing_.run_pair(it.job, next.job, err) : run_(it.job, err);
				if(rc != 0){ poison(it, rc, err); if(paired) poison(next, rc, err); }
			}
			retire(it);
			if(paired) retire(next);
			// (a waiter raised flush_waiters_ before it looked at `queued` under the lock: either it sees the new value or we see it)
			{ std::lock_guard<std::mutex> lk(m_); busy_ = false; }
			if(flush_waiters_.load(std::memory_order_seq_cst)) cv_done_.notify_all();
		}
	}

	RunFn run_; DoneFn done_; std::function<void()> on_start_; unsigned spin_us_;
	std::mutex m_; std::condition_variable cv_, cv_done_;
	std::deque<Item> q_;
	Pairing pairing_; bool has_pairing_ = false;
	std::atomic<uint32_t> n_items_{0}, flush_waiters_{0}, flush_req_{0};
	std::atomic<bool> stop_flag_{false};
	bool started_ = false, stop_ = false, worker_waiting_ = false, busy_ = false;
	std::thread th_;
};

} // namespace pcrq

#endif
