// Stand-alone check (CPU only, no library linked) of henjou-renderer_amd/host/frame_loop.hpp: render_passes, FrameWriter and ScenePrefetch
// driven with fakes.  tests/test_frame_loop_native.py builds it plain, with the address and undefined-behaviour sanitizers and with the
// thread sanitizer, and runs each; the sleeps are a few milliseconds.  Prints "frame_loop_test ok".
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "../../henjou-renderer_amd/host/frame_loop.hpp"
#include "../../henjou-renderer_amd/host/render_job.hpp"

// the one library function pass_ends calls, restated from host/capi.cpp and csrc/hjr_layout.h so that the program links nothing: a chunk of
// 8 * ceil(ceil(spp / 8) / 64) samples, or the whole frame when that is a single chunk
extern "C" uint32_t hjr_sample_granule(uint32_t spp)
{
    const uint32_t g = 8u * (((spp + 7u) / 8u + 63u) / 64u);
    return g >= spp ? spp : g;
}

static int fails = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); fails++; } } while (0)

typedef std::vector<std::pair<uint32_t, uint32_t>> Ranges; // (sample_begin, sample_end) of every launch
static void sleep_ms(int ms) { std::this_thread::sleep_for(std::chrono::milliseconds(ms)); }

// ---- render_passes
// the loop hjr_render_file had twice (its plain loop and its bucket loop), written out
static Ranges old_file_loop(uint32_t spp, uint32_t passes)
{
    const std::vector<uint32_t> ends = hjr::pass_ends(spp, passes ? passes : 1u);
    Ranges r;
    for (size_t k = 0; k < ends.size(); k++) {
        uint32_t b = 0, e = 0;
        if (ends.size() > 1) { b = k ? ends[k - 1] : 0u; e = ends[k]; }
        r.push_back({ b, e });
    }
    return r;
}
// ... and the one the rank path had.  It sent a frame of one pass as [0, spp) when the job had asked for several; the render calls read
// that range as the whole frame, [0, 0) (check_pass, csrc/hjr_render.hip), which is what `as_launched` applies
static Ranges old_rank_loop(uint32_t spp, uint32_t passes, bool as_launched)
{
    Ranges r;
    uint32_t begin = 0;
    for (const uint32_t end : hjr::pass_ends(spp, passes ? passes : 1u)) {
        if (end <= begin) continue;
        uint32_t b = 0, e = 0;
        if (passes > 1) { b = begin; e = end; }
        if (as_launched && b == 0 && e == spp) e = 0;
        r.push_back({ b, e });
        begin = end;
    }
    return r;
}
static hjr_params params_of(uint32_t spp)
{
    hjr_params p;
    HJR_INIT(p);
    p.spp = spp;
    return p;
}
static Ranges new_loop(uint32_t spp, uint32_t passes)
{
    Ranges r;
    hjr_params p = params_of(spp);
    const hjr::PassRun run = hjr::render_passes(hjr::pass_ends(spp, passes ? passes : 1u), p, passes > 1, [&](hjr_params& q) { r.push_back({ q.sample_begin, q.sample_end }); return HJR_OK; });
    CHECK(run.rc == HJR_OK && run.done == r.size() && !run.queried && !run.stopped);
    return r;
}

static void test_render_passes()
{
    // single chunk; single chunk with passes asked for; passes == 0 and 1; two passes; more passes than chunks; a last pass shorter than
    // the granule (20 spp: [0, 8) [8, 16) [16, 20)); a granule of 16; many passes
    const uint32_t table[][2] = { { 4, 1 }, { 4, 3 }, { 8, 2 }, { 16, 0 }, { 16, 1 }, { 16, 2 }, { 16, 8 }, { 20, 2 }, { 20, 5 }, { 64, 4 }, { 100, 3 }, { 600, 3 }, { 1000, 7 }, { 512, 64 } };
    for (const auto& t : table) {
        const Ranges got = new_loop(t[0], t[1]);
        if (got != old_file_loop(t[0], t[1]) || got != old_rank_loop(t[0], t[1], true)) { printf("FAILED: the launches of %u spp in %u passes changed\n", t[0], t[1]); fails++; }
    }
    CHECK((new_loop(20, 5) == Ranges{ { 0, 8 }, { 8, 16 }, { 16, 20 } }));
    CHECK((new_loop(16, 8) == Ranges{ { 0, 8 }, { 8, 16 } }));
    CHECK((new_loop(4, 3) == Ranges{ { 0, 0 } }) && (old_rank_loop(4, 3, false) == Ranges{ { 0, 4 } })); // the one place the copies differed
    CHECK((new_loop(0, 2) == Ranges{ { 0, 0 } })); // spp == 0 reaches the render call (which refuses it)
    { // a repeated end is an empty pass: skipped
        Ranges r;
        hjr_params p = params_of(16);
        const hjr::PassRun run = hjr::render_passes({ 8, 8, 16 }, p, true, [&](hjr_params& q) { r.push_back({ q.sample_begin, q.sample_end }); return HJR_OK; });
        CHECK(run.done == 2 && (r == Ranges{ { 0, 8 }, { 8, 16 } }));
    }
    // adaptive stop: no tile active after pass k, for the first, a middle and the last pass, and never
    const std::vector<uint32_t> ends = hjr::pass_ends(64, 4);
    CHECK(ends.size() == 4);
    for (const uint32_t k : { 1u, 2u, 4u, 0u }) {
        uint32_t launches = 0, queries = 0, hooks = 0;
        hjr_params p = params_of(64);
        const hjr::PassRun run = hjr::render_passes(ends, p, true, [&](hjr_params&) { launches++; return HJR_OK; },
            [&](uint32_t done) { hooks++; CHECK(done == launches && queries + 1 == launches); return HJR_OK; }, // after the launch, before the query
            [&](hjr_adaptive_state& s) { queries++; s.owned_tiles = 9; s.active_tiles = launches == k ? 0u : 5u; s.sample_end = p.sample_end; return HJR_OK; });
        const uint32_t want = k ? k : 4u;
        CHECK(run.rc == HJR_OK && launches == want && run.done == want && queries == want && hooks == want && run.queried);
        CHECK(run.stopped == (k != 0) && run.state.active_tiles == (k ? 0u : 5u) && run.state.owned_tiles == 9 && run.state.sample_end == ends[want - 1]);
        CHECK(run.state.struct_size == sizeof(hjr_adaptive_state));
    }
    { // a whole-frame launch has no adaptive state: never asked
        uint32_t queries = 0;
        hjr_params p = params_of(4);
        const hjr::PassRun run = hjr::render_passes(hjr::pass_ends(4, 3), p, true, [&](hjr_params&) { return HJR_OK; }, nullptr, [&](hjr_adaptive_state&) { queries++; return HJR_OK; });
        CHECK(run.rc == HJR_OK && run.done == 1 && queries == 0 && !run.queried && !run.stopped);
    }
    // a failure ends the frame: of the launch at pass j, of the hook, of the query
    for (const uint32_t j : { 1u, 3u, 4u }) {
        uint32_t launches = 0, hooks = 0, queries = 0;
        hjr_params p = params_of(64);
        const hjr::PassRun run = hjr::render_passes(ends, p, true, [&](hjr_params&) { return ++launches == j ? HJR_ERR_DEVICE : HJR_OK; },
            [&](uint32_t) { hooks++; return HJR_OK; }, [&](hjr_adaptive_state& s) { queries++; s.active_tiles = 1; return HJR_OK; });
        CHECK(run.rc == HJR_ERR_DEVICE && launches == j && run.done == j - 1 && hooks == j - 1 && queries == j - 1 && !run.stopped);
    }
    {
        uint32_t launches = 0, queries = 0;
        hjr_params p = params_of(64);
        hjr::PassRun run = hjr::render_passes(ends, p, true, [&](hjr_params&) { launches++; return HJR_OK; }, [&](uint32_t done) { return done == 2 ? HJR_ERR_STATE : HJR_OK; },
                                              [&](hjr_adaptive_state& s) { queries++; s.active_tiles = 1; return HJR_OK; });
        CHECK(run.rc == HJR_ERR_STATE && launches == 2 && queries == 1);
        launches = 0;
        run = hjr::render_passes(ends, p, true, [&](hjr_params&) { launches++; return HJR_OK; }, nullptr, [&](hjr_adaptive_state&) { return HJR_ERR_ARG; });
        CHECK(run.rc == HJR_ERR_ARG && launches == 1 && !run.queried && !run.stopped);
    }
}

// ---- FrameWriter
static const size_t FLOATS = 1024;
static float pattern(int frame, size_t j) { return (float)(frame * 4096 + (int)j); }

struct WriterRun {
    std::vector<std::string> seen;          // the names the sink got, in its order
    std::vector<std::thread::id> sink_threads;
    int max_outstanding = 0, bad_patterns = 0;
    std::vector<std::pair<int, std::string>> reports; // every error an operation gave the producer
};
// 7 frames, so each slot is used at least three times; the sink sleeps 1 - 4 ms, the producer 0 - 2 ms; frames in `failing` fail in the sink
static WriterRun writer_run(bool serial, const std::vector<int>& failing, bool drain)
{
    WriterRun w;
    std::atomic<int> submitted{ 0 }, finished{ 0 };
    {
        hjr::FrameWriter fw(FLOATS, [&](const float* rgba, const std::string& name, std::string& err) {
            const int frame = (int)w.seen.size(), out = submitted.load() - finished.load();
            if (out > w.max_outstanding) w.max_outstanding = out;
            w.seen.push_back(name);
            w.sink_threads.push_back(std::this_thread::get_id());
            for (int round = 0; round < 2; round++) { // the slot is the sink's until it returns: intact before and after the sleep
                for (size_t j = 0; j < FLOATS; j++) if (rgba[j] != pattern(frame, j)) { w.bad_patterns++; break; }
                if (round == 0) sleep_ms(1 + frame * 3 % 4);
            }
            finished++;
            for (const int f : failing) if (f == frame) { err = "cannot write " + name; return HJR_ERR_IO; }
            return HJR_OK;
        }, serial);
        std::string err;
        for (int frame = 0; frame < 7; frame++) {
            float* buf = nullptr;
            int rc = fw.acquire(buf, err);
            if (rc != HJR_OK) w.reports.push_back({ rc, err }); // (a driver stops here; this one goes on: later frames are still consumed)
            for (size_t j = 0; j < FLOATS; j++) buf[j] = pattern(frame, j);
            sleep_ms(frame % 3);
            submitted++;
            rc = fw.submit("f" + std::to_string(frame), err);
            if (rc != HJR_OK) w.reports.push_back({ rc, err });
        }
        if (drain) {
            const int rc = fw.drain(err);
            if (rc != HJR_OK) w.reports.push_back({ rc, err });
            CHECK(finished.load() == 7);                // drain returned with everything written
            CHECK(fw.drain(err) == HJR_OK);             // ... and may be called again
        }
    } // (the destructor joins: `w` is the producer's again)
    return w;
}

static void test_frame_writer()
{
    const std::vector<std::string> names = { "f0", "f1", "f2", "f3", "f4", "f5", "f6" };
    for (const bool serial : { false, true }) {
        WriterRun w = writer_run(serial, {}, true);
        CHECK(w.seen == names && w.bad_patterns == 0 && w.reports.empty());
        CHECK(w.max_outstanding >= 1 && w.max_outstanding <= (serial ? 1 : 2));
        for (const std::thread::id id : w.sink_threads) CHECK((id == std::this_thread::get_id()) == serial); // serial: no thread
        // the sink fails on frame 3, and again on frame 5: the producer is told once, frame 3's error, and every frame is still consumed
        w = writer_run(serial, { 3, 5 }, true);
        CHECK(w.seen == names && w.bad_patterns == 0);
        CHECK(w.reports.size() == 1 && w.reports[0].first == HJR_ERR_IO && w.reports[0].second == "cannot write f3");
        // no drain: the destructor neither hangs nor ends the program, and the submitted frames are written
        w = writer_run(serial, { 6 }, false);
        CHECK(w.seen == names && w.bad_patterns == 0 && (w.reports.empty() || serial));
    }
    { // nothing submitted
        hjr::FrameWriter fw(FLOATS, [](const float*, const std::string&, std::string&) { return HJR_OK; }, false);
    }
}

// ---- ScenePrefetch
static thread_local std::string tl_error = "nothing yet"; // stands for hjr_last_error(): per thread

static void test_scene_prefetch()
{
    for (const bool serial : { false, true }) {
        tl_error = "the caller's own text";
        uint32_t calls = 0;
        std::thread::id ran_on;
        std::atomic<bool> finished{ false };
        auto prepare = [&](uint32_t frame) {
            calls++;
            ran_on = std::this_thread::get_id();
            sleep_ms(3);
            finished = true;
            if (frame % 2 == 0) return HJR_OK;
            tl_error = "frame " + std::to_string(frame) + " cannot be prepared";
            return HJR_ERR_DEVICE;
        };
        auto last_error = [] { return tl_error; };
        std::string err = "untouched";
        {
            hjr::ScenePrefetch sp(prepare, last_error, serial);
            CHECK(sp.take(err) == HJR_OK && err == "untouched"); // nothing started
            CHECK(sp.start(4) == HJR_OK);
            CHECK(sp.start(6) == HJR_ERR_STATE); // one update at a time: refused, nothing started
            CHECK(sp.take(err) == HJR_OK && err == "untouched" && calls == 1 && finished);
            CHECK((ran_on == std::this_thread::get_id()) == serial);
            CHECK(sp.take(err) == HJR_OK); // a result is taken once
            CHECK(sp.start(7) == HJR_OK);
            CHECK(sp.take(err) == HJR_ERR_DEVICE && err == "frame 7 cannot be prepared" && calls == 2);
            if (!serial) CHECK(tl_error == "the caller's own text"); // the text came over from the helper thread
            CHECK(sp.start(8) == HJR_OK && sp.take(err) == HJR_OK && calls == 3); // usable after a failure
            finished = false;
            CHECK(sp.start(10) == HJR_OK);
        } // the destructor joins
        CHECK(finished && calls == 4);
    }
}

int main()
{
    test_render_passes();
    test_frame_writer();
    test_scene_prefetch();
    if (fails) { printf("frame_loop_test: %d check(s) failed\n", fails); return 1; }
    printf("frame_loop_test ok\n");
    return 0;
}
