// An ordered launcher: a FIFO of jobs served by ONE thread, shared by several producers ("clients": the library's handles on one
// stream).  The thread is created by the first push and joined by stop(); between jobs it spins on the queue for a bounded time and
// then blocks on a condition variable.  No HIP here: the jobs are opaque, the owner passes what runs them (tested on the CPU,
// tests/launch_queue_check.cpp).
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
		const auto t_end = std::chrono::steady_clock::now() + std::chrono::microseconds(200);
		while(std::chrono::steady_clock::now() < t_end){
			if(c->queued.load(std::memory_order_seq_cst) == 0) return;
			cpu_relax();
		}
		flush_waiters_.fetch_add(1, std::memory_order_seq_cst);
		{
			std::unique_lock<std::mutex> lk(m_);
			cv_done_.wait(lk, [&]{ return c->queued.load(std::memory_order_seq_cst) == 0; });
		}
		flush_waiters_.fetch_sub(1, std::memory_order_seq_cst);
	}
	// returns when the queue holds no job and none is running
	void wait_empty()
	{
		flush_waiters_.fetch_add(1, std::memory_order_seq_cst);
		{
			std::unique_lock<std::mutex> lk(m_);
			cv_done_.wait(lk, [&]{ return q_.empty() && !busy_; });
		}
		flush_waiters_.fetch_sub(1, std::memory_order_seq_cst);
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
	void work()
	{
		if(on_start_) on_start_();
		Item it;
		while(pop(it)){
			Client *const c = it.client;
			if(!stop_flag_.load(std::memory_order_acquire) && !c->poisoned.load(std::memory_order_acquire)){
				std::string err;
				const int rc = run_(it.job, err);
				if(rc != 0){
					c->err_code = rc; c->err_msg = err; c->err_tag = it.tag;
					c->poisoned.store(true, std::memory_order_release);
				}
			}
			done_(it.job);
			c->queued.fetch_sub(1, std::memory_order_seq_cst);
			// (a waiter raised flush_waiters_ before it looked at `queued` under the lock: either it sees the new value or we see it)
			{ std::lock_guard<std::mutex> lk(m_); busy_ = false; }
			if(flush_waiters_.load(std::memory_order_seq_cst)) cv_done_.notify_all();
		}
	}

	RunFn run_; DoneFn done_; std::function<void()> on_start_; unsigned spin_us_;
	std::mutex m_; std::condition_variable cv_, cv_done_;
	std::deque<Item> q_;
	std::atomic<uint32_t> n_items_{0}, flush_waiters_{0};
	std::atomic<bool> stop_flag_{false};
	bool started_ = false, stop_ = false, worker_waiting_ = false, busy_ = false;
	std::thread th_;
};

} // namespace pcrq

#endif
