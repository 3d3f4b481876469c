// ---- shard workers (single-process multi-device) ----------------------------
// A kernel launch costs the host 3 - 4 us (MI355X_MICROARCH.md), so eight launches issued one
// after the other from the calling thread cost more than the 13 us a 2048-world shard renders
// in: the one-Manager form every reference caller uses (/root/reference/scripts/test.py:112-130,
// one ctor, one step()) would be host-bound at 8 devices.  Each shard but the first therefore
// has a host thread of its own, created by mrx_create, bound to its device once, parked on a
// command word.  mrx_step stores the next command word into every worker's word, launches
// shard 0 itself and waits until every worker has acknowledged -- when it returns, every
// device has the kernel in its queue (a caller's next operation on those streams is ordered
// behind it, exactly as in the serial form), and the host paid for one launch plus a cache-line
// handshake.  Workers spin on their word for a while after a command (a simulation loop calls
// step() every few tens of microseconds) and then sleep in a futex; MRX_SHARD_SPIN_US sets how
// long (default 200), MRX_SHARD_THREADS=0 restores the serial form (startShardWorkers).
//
// The command word: sequence number in the high 24 bits, command in the low 8 (commandWord).  A worker takes the
// command out of the very word whose change woke it, so it never runs a command under another post's sequence
// number, and it acknowledges with the same word.  Consecutive words differ in their sequence bits, so "changed" is
// a plain inequality; the sequence wraps modulo 2^24, and a worker is never that far behind: every command but a
// counted render is acknowledged before the next is posted, and counted renders run at most 256 ahead.  `steps` is
// written before the word is released and read after it is acquired; the master cannot post another command with
// `steps` before this one is acknowledged.
#include "shards.hpp"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <thread>

#include <linux/futex.h>
#include <sys/syscall.h>
#include <unistd.h>

#include "../../include/mrx.h"
#include "error.hpp"

struct ShardWorker {
    ShardGroup shards;                          // the shards of ONE device, launched in order
    ShardBindFn bind = nullptr;
    ShardRunFn run = nullptr;
    int64_t spinNs = 0;                         // MRX_SHARD_SPIN_US
    std::thread th;
    // written by the master, read by the worker
    alignas(64) std::atomic<uint32_t> posted { 0 };     // the command word
    int steps = 0;                              // (ordered by `posted`)
    alignas(64) std::atomic<uint32_t> sleeping { 0 };
    // written by the worker, read by the master
    alignas(64) std::atomic<uint32_t> done { 0 };
    int rc = MRX_OK;
    std::string err;
    int64_t tSeen = 0, tDone = 0;               // MRX_SHARD_TRACE: when the command was seen / finished
    alignas(64) std::atomic<uint32_t> masterSleeping { 0 };
    // MRX_SHARD_ASYNC=1: renders are counted, not acknowledged one by one -- the caller posts (renderPosted)
    // and goes on, the worker launches until it has caught up (renderDone); every other command joins first
    bool async = false;
    alignas(64) std::atomic<uint32_t> renderPosted { 0 };
    alignas(64) std::atomic<uint32_t> renderDone { 0 };
};

namespace {

constexpr uint32_t kCmdBits = 8;
inline uint32_t commandWord(uint32_t seq, int cmd) { return seq << kCmdBits | (uint32_t)cmd; }
inline int commandOf(uint32_t word) { return (int)(word & ((1u << kCmdBits) - 1u)); }

inline void cpuRelax() { __builtin_ia32_pause(); }

inline long futexWait(std::atomic<uint32_t> *word, uint32_t expected)
{
    return syscall(SYS_futex, reinterpret_cast<uint32_t *>(word), FUTEX_WAIT_PRIVATE, expected, nullptr, nullptr, 0);
}

inline long futexWake(std::atomic<uint32_t> *word)
{
    return syscall(SYS_futex, reinterpret_cast<uint32_t *>(word), FUTEX_WAKE_PRIVATE, INT_MAX, nullptr, nullptr, 0);
}

bool shardTrace()
{
    static const bool on = std::getenv("MRX_SHARD_TRACE") != nullptr;
    return on;
}

// MRX_SHARD_TRACE: sums over the render commands of a renderer (ns): post -> worker saw it (worst
// worker), the worker's launch (worst), the calling thread's own launch, post -> all acknowledged
struct ShardTrace { int64_t wake = 0, launch = 0, own = 0, total = 0, n = 0; };
thread_local ShardTrace g_trace;

int64_t nowNs()
{
    return std::chrono::duration_cast<std::chrono::nanoseconds>(
               std::chrono::steady_clock::now().time_since_epoch()).count();
}

void shardWorkerMain(ShardWorker *w)
{
    const int bound = w->bind(w->shards);
    const std::string boundErr = bound != MRX_OK ? g_err : std::string();
    uint32_t seen = 0;
    int64_t lastWork = nowNs();
    for (;;) {
        uint32_t word;
        // park: spin while commands keep coming, then sleep
        for (uint32_t it = 0;; ++it) {
            word = w->posted.load(std::memory_order_acquire);
            if (word != seen)
                break;
            if ((it & 255u) == 255u && nowNs() - lastWork > w->spinNs) {
                w->sleeping.store(1, std::memory_order_seq_cst);
                if (w->posted.load(std::memory_order_seq_cst) == seen)
                    futexWait(&w->posted, seen);
                w->sleeping.store(0, std::memory_order_relaxed);
                continue;
            }
            cpuRelax();
        }
        seen = word;
        const int cmd = commandOf(word);
        if (shardTrace())
            w->tSeen = nowNs();
        if (w->async) {
            // counted renders: launch until caught up (a failure is kept for the next join and the
            // count still advances, so that nobody waits for a launch that will not come)
            uint32_t doneR = w->renderDone.load(std::memory_order_relaxed);
            while (doneR != w->renderPosted.load(std::memory_order_acquire)) {
                int rc = bound == MRX_OK ? w->run(w->shards, kCmdRender, 0, false) : fail(bound, boundErr);
                if (rc != MRX_OK && w->rc == MRX_OK) {
                    w->err = g_err;
                    w->rc = rc;
                }
                w->renderDone.store(++doneR, std::memory_order_release);
            }
            lastWork = nowNs();
            if (cmd == kCmdRender)
                continue;                             // (nothing to acknowledge: the count is the acknowledgement)
        }
        if (cmd == kCmdExit) {
            w->done.store(word, std::memory_order_release);
            return;
        }
        int rc = MRX_OK;
        if (bound != MRX_OK)
            rc = fail(bound, boundErr);
        if (rc == MRX_OK)
            rc = w->run(w->shards, cmd, w->steps, false);
        if (!(w->async && w->rc != MRX_OK)) {         // (an error of a counted render waits for its join)
            w->rc = rc;
            if (rc != MRX_OK)
                w->err = g_err;
        }
        if (shardTrace())
            w->tDone = nowNs();
        w->done.store(word, std::memory_order_seq_cst);
        if (w->masterSleeping.load(std::memory_order_seq_cst))
            futexWake(&w->done);
        lastWork = nowNs();
    }
}

void post(ShardWorker *w, uint32_t word)
{
    w->posted.store(word, std::memory_order_seq_cst);
    if (w->sleeping.load(std::memory_order_seq_cst))
        futexWake(&w->posted);
}

}  // namespace

// MRX_SHARD_ASYNC: wait until every device thread has enqueued every render posted so far; the
// first failure among them is reported here (and cleared)
int joinRenders(ShardSet &s)
{
    if (!s.shardAsync)
        return MRX_OK;
    int rc = MRX_OK;
    std::string err;
    for (ShardWorker *w : s.workers) {
        for (uint32_t it = 0; w->renderDone.load(std::memory_order_acquire) != s.rendersPosted; ++it) {
            if ((it & 1023u) == 1023u)
                std::this_thread::yield();
            else
                cpuRelax();
        }
        if (w->rc != MRX_OK) {
            if (rc == MRX_OK) {
                rc = w->rc;
                err = w->err;
            }
            w->rc = MRX_OK;
        }
    }
    return rc == MRX_OK ? MRX_OK : fail(rc, err);
}

// run `cmd` on every shard of a multi-device renderer: workers in parallel, shard 0 (and any
// shard without a worker) on the calling thread; returns the first failure
int shardsRun(ShardSet &s, int cmd, int steps)
{
    if (s.shardAsync) {
        if (cmd == kCmdRender) {
            // post and go on; at most 256 renders ahead of the slowest device thread
            const uint32_t n = ++s.rendersPosted;
            const uint32_t word = commandWord(++s.workerSeq, kCmdRender);
            for (ShardWorker *w : s.workers) {
                while (n - w->renderDone.load(std::memory_order_acquire) > 256u)
                    cpuRelax();
                w->renderPosted.store(n, std::memory_order_release);
                post(w, word);
            }
            return MRX_OK;
        }
        const int jrc = joinRenders(s);
        if (jrc != MRX_OK)
            return jrc;
    }
    const uint32_t word = commandWord(++s.workerSeq, cmd);
    const bool trace = shardTrace() && cmd == kCmdRender;
    const int64_t tPost = trace ? nowNs() : 0;
    int64_t tOwn = 0;
    for (ShardWorker *w : s.workers) {
        w->steps = steps;
        post(w, word);
    }
    int rc = s.run(s.ownShards, cmd, steps, true);
    if (trace)
        tOwn = nowNs();
    std::string err = rc != MRX_OK ? g_err : std::string();
    for (ShardWorker *w : s.workers) {
        // an enqueue takes microseconds: spin; a stream synchronisation may take long: sleep
        const int64_t t0 = nowNs();
        for (uint32_t it = 0; w->done.load(std::memory_order_acquire) != word; ++it) {
            if ((it & 255u) == 255u && nowNs() - t0 > 50000) {
                w->masterSleeping.store(1, std::memory_order_seq_cst);
                const uint32_t cur = w->done.load(std::memory_order_seq_cst);
                if (cur != word)
                    futexWait(&w->done, cur);
                w->masterSleeping.store(0, std::memory_order_relaxed);
                continue;
            }
            cpuRelax();
        }
        if (w->rc != MRX_OK) {
            if (rc == MRX_OK) {
                rc = w->rc;
                err = w->err;
            }
            w->rc = MRX_OK;                           // (consumed: the next join does not report it again)
        }
    }
    if (trace) {
        int64_t wake = 0, launch = 0;
        for (ShardWorker *w : s.workers) {
            wake = std::max(wake, w->tSeen - tPost);
            launch = std::max(launch, w->tDone - w->tSeen);
        }
        g_trace.wake += wake;
        g_trace.launch += launch;
        g_trace.own += tOwn - tPost;
        g_trace.total += nowNs() - tPost;
        g_trace.n++;
    }
    if (rc != MRX_OK)
        return fail(rc, err);
    return MRX_OK;
}

void startShardWorkers(ShardSet &s, const ShardGroup &shards, const std::vector<int> &devices, bool asyncFlag,
                       ShardBindFn bind, ShardRunFn run)
{
    // One host thread per DEVICE: shards that share a device share its queues and (by default)
    // its null stream, where concurrent launches only queue up behind the runtime's stream lock
    // (profiles/r04_multidev_host.txt: eight threads on one null stream 48 us per step against
    // 32 us from one thread).  The first device's shards stay with the calling thread.
    // MRX_SHARD_THREADS=0: no threads at all; =2: a thread per shard whatever its device (the
    // one-GPU rehearsal of a node, with a stream per shard).
    int mode = 1;
    if (const char *e = std::getenv("MRX_SHARD_THREADS"))
        mode = std::atoi(e);
    if (mode <= 0)
        return;
    std::vector<ShardGroup> groups;
    std::vector<int> groupDevice;
    for (size_t i = 0; i < shards.size(); ++i) {
        bool placed = false;
        for (size_t g = 0; g < groups.size() && !placed; ++g)
            if (mode == 1 && groupDevice[g] == devices[i]) {
                groups[g].push_back(shards[i]);
                placed = true;
            }
        if (!placed) {
            groups.push_back({ shards[i] });
            groupDevice.push_back(devices[i]);
        }
    }
    if (groups.size() <= 1)
        return;
    // MRX_SHARD_ASYNC=1 (opt-in): mrx_step only POSTS the render -- every device, the first included, has a
    // thread -- and returns; the threads enqueue behind its back, and every other mrx_* call on the renderer or
    // on one of its shards joins them first (mrx_sync, mrx_buffer ..., the next non-render command).  The host
    // pays a cache line per device for a step, not a launch.  What the caller gives up: an operation it enqueues
    // ITSELF on a shard's stream right after mrx_step (a torch kernel on tensors fetched earlier) is no longer
    // ordered behind the render unless an mrx_* call came in between.
    s.shardAsync = asyncFlag;
    if (const char *e = std::getenv("MRX_SHARD_ASYNC"))
        s.shardAsync = std::atoi(e) != 0;
    s.run = run;
    const char *spin = std::getenv("MRX_SHARD_SPIN_US");
    const size_t firstWorker = s.shardAsync ? 0 : 1;
    if (!s.shardAsync)
        s.ownShards = groups[0];
    for (size_t g = firstWorker; g < groups.size(); ++g) {
        ShardWorker *w = new ShardWorker();
        w->shards = groups[g];
        w->bind = bind;
        w->run = run;
        w->spinNs = (int64_t)(spin ? std::max(0, std::atoi(spin)) : 200) * 1000;
        w->async = s.shardAsync;
        w->th = std::thread(shardWorkerMain, w);
        s.workers.push_back(w);
    }
}

void stopShardWorkers(ShardSet &s)
{
    if (s.workers.empty())
        return;
    const uint32_t word = commandWord(++s.workerSeq, kCmdExit);
    for (ShardWorker *w : s.workers) {
        w->posted.store(word, std::memory_order_seq_cst);
        futexWake(&w->posted);
    }
    for (ShardWorker *w : s.workers) {
        w->th.join();
        delete w;
    }
    s.workers.clear();
}

void shardTraceReset() { g_trace = ShardTrace {}; }

void shardTraceReport()
{
    if (shardTrace() && g_trace.n) {
        const double n = (double)g_trace.n * 1000.0;
        std::fprintf(stderr, "mrx shard trace (%lld steps, us): wake %.2f  worker launch %.2f  own launch %.2f  all enqueued %.2f\n",
                     (long long)g_trace.n, g_trace.wake / n, g_trace.launch / n, g_trace.own / n, g_trace.total / n);
        g_trace = ShardTrace {};
    }
}
