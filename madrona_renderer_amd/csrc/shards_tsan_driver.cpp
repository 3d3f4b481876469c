// ThreadSanitizer driver of the shard-worker protocol (shards.cpp), built by `python -m madrona_renderer_amd.build
// --shards-driver` with the host compiler only and run by tests/test_sanitizers.py on the CPU.  No HIP: a shard is a
// record of plain counters, the run callback counts what each shard was told to do.  The counters are NOT atomic on
// purpose -- the master reads them after a command returned or a join passed, so ThreadSanitizer also checks that the
// protocol orders a worker's effects before the caller's next step.  Every scenario checks exact counts; a report or a
// wrong count ends the run with a non-zero status.
//   shards_tsan_driver [pairing rounds, default 10000]
#include "shards.hpp"

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <thread>

#include "../../include/mrx.h"
#include "error.hpp"

struct mrx_renderer {
    int id = 0;
    long renders = 0;                           // kCmdRender calls plus the steps of every kCmdTimed
    long timedBegin = 0, timedEnd = 0;          // kCmdTimed: its prologue and epilogue
    long syncs = 0, stage[4] = {}, other = 0;
    long unbound = 0;                           // calls that came with bindDevice set
};

namespace {

// what the stub is told (written by the master before it posts; read by whichever thread runs the command)
int g_failShard = -1, g_failCmd = 0;
long g_failRenderAt = 0;                        // the n-th render of g_failShard fails (1-based)
int g_sleepUs = 0;                              // every render takes this long
int g_bindFailFrom = -1;                        // groups whose first shard has id >= this fail to bind

int stubRun(const ShardGroup &group, int cmd, int steps, bool bindDevice)
{
    for (mrx_renderer *sh : group) {
        sh->unbound += bindDevice ? 1 : 0;
        if (cmd == kCmdRender) {
            ++sh->renders;
            if (g_sleepUs)
                std::this_thread::sleep_for(std::chrono::microseconds(g_sleepUs));
            if (sh->id == g_failShard && sh->renders == g_failRenderAt)
                return fail(MRX_E_HIP, "stub: render " + std::to_string(sh->renders) + " of shard " + std::to_string(sh->id));
        } else if (cmd == kCmdTimed) {
            ++sh->timedBegin;
            sh->renders += steps;
            ++sh->timedEnd;
        } else if (cmd == kCmdSync) {
            ++sh->syncs;
        } else if (cmd >= kCmdStage && cmd < kCmdStage + 4) {
            ++sh->stage[cmd - kCmdStage];
            if (sh->id == g_failShard && cmd == g_failCmd)
                return fail(MRX_E_HIP, "stub: stage of shard " + std::to_string(sh->id));
        } else {
            ++sh->other;
        }
    }
    return MRX_OK;
}

int stubBind(const ShardGroup &group)
{
    if (g_bindFailFrom >= 0 && group[0]->id >= g_bindFailFrom)
        return fail(MRX_E_HIP, "stub: no device for shard " + std::to_string(group[0]->id));
    return MRX_OK;
}

int g_checks = 0;
#define CHECK(cond)                                                                              \
    do {                                                                                         \
        ++g_checks;                                                                              \
        if (!(cond)) {                                                                           \
            std::fprintf(stderr, "FAILED %s:%d (%s): %s\n", __FILE__, __LINE__, what, #cond);    \
            std::exit(1);                                                                        \
        }                                                                                        \
    } while (0)

// a renderer's worth of shards on the given devices, its workers started under the given switches
struct Job {
    std::vector<mrx_renderer> recs;
    ShardGroup shards;
    ShardSet set;
    Job(const std::vector<int> &devices, bool async, int spinUs, const char *threads = "1")
    {
        setenv("MRX_SHARD_ASYNC", async ? "1" : "0", 1);
        setenv("MRX_SHARD_SPIN_US", std::to_string(spinUs).c_str(), 1);
        setenv("MRX_SHARD_THREADS", threads, 1);
        recs.resize(devices.size());
        for (size_t i = 0; i < recs.size(); ++i) {
            recs[i].id = (int)i;
            shards.push_back(&recs[i]);
        }
        startShardWorkers(set, shards, devices, false, stubBind, stubRun);
    }
    ~Job() { stopShardWorkers(set); }
};

void sleepUs(int us) { std::this_thread::sleep_for(std::chrono::microseconds(us)); }

// bursts, idle gaps, a stage command; every shard must have been told exactly what was posted
void scenarioCounts(const char *what, const std::vector<int> &devices, size_t groups, bool async, int spinUs,
                    const char *threads = "1")
{
    Job j(devices, async, spinUs, threads);
    CHECK(j.set.shardAsync == async);
    CHECK(j.set.workers.size() == (async ? groups : groups - 1));
    const long burst = 3000, gaps = 12;
    for (long i = 0; i < burst; ++i)
        CHECK(shardsRun(j.set, kCmdRender) == MRX_OK);
    CHECK(shardsRun(j.set, kCmdSync) == MRX_OK);
    for (const mrx_renderer &sh : j.recs)
        CHECK(sh.renders == burst && sh.syncs == 1);
    // workers asleep in the futex between renders
    for (long i = 0; i < gaps; ++i) {
        sleepUs(spinUs * 4 + 300);
        CHECK(shardsRun(j.set, kCmdRender) == MRX_OK);
    }
    sleepUs(spinUs * 4 + 300);
    CHECK(shardsRun(j.set, kCmdStage + 2) == MRX_OK);
    CHECK(joinRenders(j.set) == MRX_OK);
    for (const mrx_renderer &sh : j.recs) {
        CHECK(sh.renders == burst + gaps && sh.stage[2] == 1 && sh.stage[0] + sh.stage[1] + sh.stage[3] == 0);
        CHECK(sh.timedBegin == 0 && sh.other == 0);
    }
    // the calling thread's own shards come with bindDevice set, a worker's never
    long unbound = 0;
    for (const mrx_renderer &sh : j.recs)
        unbound += sh.unbound;
    if (async) {
        CHECK(unbound == 0);
    } else {
        CHECK(unbound == (long)j.set.ownShards.size() * (burst + gaps + 2));
    }
}

// MRX_SHARD_ASYNC: two renders, at once a timed command of k steps, a sync -- per round every shard renders exactly
// 2 + k times and sees the timed prologue and epilogue once (a command run under another post's sequence number would
// run twice)
void scenarioPairing(const char *what, int spinUs, long rounds)
{
    Job j({ 0, 1, 1, 2 }, true, spinUs);
    for (long r = 0; r < rounds; ++r) {
        const int k = 1 + (int)(r % 3);
        CHECK(shardsRun(j.set, kCmdRender) == MRX_OK);
        CHECK(shardsRun(j.set, kCmdRender) == MRX_OK);
        CHECK(shardsRun(j.set, kCmdTimed, k) == MRX_OK);
        CHECK(shardsRun(j.set, kCmdSync) == MRX_OK);
        for (mrx_renderer &sh : j.recs) {
            if (sh.renders != 2 + k || sh.timedBegin != 1 || sh.timedEnd != 1 || sh.syncs != 1)
                std::fprintf(stderr, "round %ld shard %d: %ld renders (want %d), timed %ld / %ld, %ld syncs\n", r, sh.id,
                             sh.renders, 2 + k, sh.timedBegin, sh.timedEnd, sh.syncs);
            CHECK(sh.renders == 2 + k && sh.timedBegin == 1 && sh.timedEnd == 1 && sh.syncs == 1);
            sh.renders = sh.timedBegin = sh.timedEnd = sh.syncs = 0;
        }
    }
}

void scenarioFailures(const char *what)
{
    {   // async: a failing render surfaces at the next join and only there
        Job j({ 0, 1, 2 }, true, 50);
        g_failShard = 1;
        g_failRenderAt = 2;
        for (int i = 0; i < 3; ++i)
            CHECK(shardsRun(j.set, kCmdRender) == MRX_OK);
        CHECK(joinRenders(j.set) == MRX_E_HIP);
        CHECK(g_err == "stub: render 2 of shard 1");
        CHECK(joinRenders(j.set) == MRX_OK);
        CHECK(shardsRun(j.set, kCmdSync) == MRX_OK);
        for (const mrx_renderer &sh : j.recs)
            CHECK(sh.renders == 3 && sh.syncs == 1);     // (the count advances past a failure)
        // ... and a command that finds a failed render behind it reports that instead of running
        g_failRenderAt = 4;
        CHECK(shardsRun(j.set, kCmdRender) == MRX_OK);
        CHECK(shardsRun(j.set, kCmdSync) == MRX_E_HIP);
        CHECK(g_err == "stub: render 4 of shard 1");
        CHECK(shardsRun(j.set, kCmdSync) == MRX_OK);
        // async: a failing command that is no render is reported by its call, not again by the next join
        g_failCmd = kCmdStage + 1;
        CHECK(shardsRun(j.set, kCmdStage + 1) == MRX_E_HIP);
        CHECK(g_err == "stub: stage of shard 1");
        CHECK(joinRenders(j.set) == MRX_OK);
        CHECK(shardsRun(j.set, kCmdRender) == MRX_OK);
        CHECK(joinRenders(j.set) == MRX_OK);
        g_failShard = -1;
    }
    {   // sync: a failing command of a worker's shard, and of the caller's own, is reported once by that call
        Job j({ 0, 1, 2 }, false, 50);
        g_failCmd = kCmdStage + 1;
        for (int shard : { 2, 0 }) {
            g_failShard = shard;
            CHECK(shardsRun(j.set, kCmdStage + 1) == MRX_E_HIP);
            CHECK(g_err == "stub: stage of shard " + std::to_string(shard));
            g_failShard = -1;
            CHECK(shardsRun(j.set, kCmdStage + 1) == MRX_OK);
            CHECK(shardsRun(j.set, kCmdRender) == MRX_OK);
        }
        g_failCmd = 0;
    }
    for (bool async : { false, true }) {   // a worker that cannot bind its device says so on every command
        g_bindFailFrom = 1;
        Job j({ 0, 1 }, async, 50);
        for (int i = 0; i < 3; ++i) {
            const int rc = shardsRun(j.set, kCmdRender);
            CHECK(rc == (async ? MRX_OK : MRX_E_HIP));
            CHECK(shardsRun(j.set, kCmdSync) == MRX_E_HIP);
            CHECK(g_err == "stub: no device for shard 1");
        }
        CHECK(j.recs[1].renders == 0 && j.recs[1].syncs == 0);
        g_bindFailFrom = -1;
    }
}

void scenarioStop(const char *what)
{
    for (bool async : { false, true })
        for (int spinUs : { 0, 50 }) {
            {   // stop while the workers sleep
                Job j({ 0, 1, 2 }, async, spinUs);
                CHECK(shardsRun(j.set, kCmdRender) == MRX_OK);
                sleepUs(spinUs * 4 + 500);
            }
            // stop right after a post: what was posted still runs
            Job j({ 0, 1, 2 }, async, spinUs);
            g_sleepUs = 20;
            for (int i = 0; i < 5; ++i)
                CHECK(shardsRun(j.set, kCmdRender) == MRX_OK);
            stopShardWorkers(j.set);
            g_sleepUs = 0;
            CHECK(j.set.workers.empty());
            for (const mrx_renderer &sh : j.recs)
                CHECK(sh.renders == 5);
        }
    // no threads where none are wanted
    {
        Job j({ 0, 1, 2 }, false, 50, "0");
        CHECK(j.set.workers.empty());
    }
    Job j({ 3, 3, 3 }, true, 50);
    CHECK(j.set.workers.empty() && !j.set.shardAsync);
}

}  // namespace

int main(int argc, char **argv)
{
    const long rounds = argc > 1 ? std::atol(argv[1]) : 10000;
    for (bool async : { false, true })
        for (int spinUs : { 0, 50 }) {
            scenarioCounts("2 groups", { 0, 1 }, 2, async, spinUs);
            scenarioCounts("3 groups", { 0, 1, 2 }, 3, async, spinUs);
            scenarioCounts("8 groups", { 0, 1, 2, 3, 4, 5, 6, 7 }, 8, async, spinUs);
            scenarioCounts("shards sharing a group", { 0, 0, 1, 2, 1 }, 3, async, spinUs);
            scenarioCounts("a thread per shard", { 0, 0, 1 }, 3, async, spinUs, "2");
        }
    for (int spinUs : { 0, 50 })
        scenarioPairing("pairing", spinUs, rounds);
    scenarioFailures("failures");
    scenarioStop("stop");
    std::printf("shards: %d checks, %ld pairing rounds per spin setting, all passed\n", g_checks, rounds);
    return 0;
}
