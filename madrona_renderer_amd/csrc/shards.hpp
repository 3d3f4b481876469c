// The shard-worker protocol (shards.cpp): the host threads that run a multi-device renderer's commands, one per
// device.  No HIP and no renderer in here: a shard is an opaque handle, and what a command does to the shards of one
// device is the caller's run callback.  A failure's text travels in the shared fail / g_err (error.hpp).
#pragma once

#include <cstdint>
#include <vector>

#pragma GCC visibility push(hidden)

// what a worker can be told; kCmdStage + i: run post-render stage i on every shard of the group
enum : int { kCmdNone = 0, kCmdRender, kCmdSync, kCmdTimed, kCmdObserveRestart, kCmdExit, kCmdStage };

struct mrx_renderer;                            // (the C ABI's handle: never looked into here)
using ShardGroup = std::vector<mrx_renderer *>; // the shards of ONE device, launched in order
// what the shards of a group do for a command, on whichever thread runs it: an MRX_* code, its text in g_err.
// bindDevice: the thread is not bound to the group's device for good, make it current first
using ShardRunFn = int (*)(const ShardGroup &group, int cmd, int steps, bool bindDevice);
// once on a worker's thread, before its first command: bind the thread to the group's device.  A failure (an MRX_*
// code, its text in g_err) is what every command of that worker then reports
using ShardBindFn = int (*)(const ShardGroup &group);

struct ShardWorker;

// the protocol's state in a multi-device renderer
struct ShardSet {
    // one persistent host thread per device but the first (whose shards the calling thread
    // launches): mrx_step posts the launch to all of them and returns when every device has its
    // kernel enqueued -- the host cost of a step is the slowest enqueue, not their sum
    std::vector<ShardWorker *> workers;
    ShardGroup ownShards;                       // (with workers) the shards the calling thread launches
    uint32_t workerSeq = 0;
    bool shardAsync = false;                    // MRX_SHARD_ASYNC=1 (startShardWorkers)
    uint32_t rendersPosted = 0;
    ShardRunFn run = nullptr;
};

// shards[i] lives on devices[i]; asyncFlag: MRX_FLAG_SHARD_ASYNC of the renderer.  Leaves `s` without workers where
// the commands are to run from the calling thread (MRX_SHARD_THREADS=0, a single group)
void startShardWorkers(ShardSet &s, const ShardGroup &shards, const std::vector<int> &devices, bool asyncFlag,
                       ShardBindFn bind, ShardRunFn run);
void stopShardWorkers(ShardSet &s);
// (a set with workers) run `cmd` on every group: workers in parallel, the own shards on the calling thread
int shardsRun(ShardSet &s, int cmd, int steps = 0);
int joinRenders(ShardSet &s);

// MRX_SHARD_TRACE, for mrx_time_steps_host: forget the calling thread's sums / print them to stderr and forget them
void shardTraceReset();
void shardTraceReport();

#pragma GCC visibility pop
