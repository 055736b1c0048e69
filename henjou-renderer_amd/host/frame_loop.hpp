// The frame loop shared by the two drivers of a render_option.json (hjr_render_file in host/render_file.cpp, the rank path of
// cli/henjou_cli.cpp): the one loop over a frame's sample passes, the two-slot output stage and the helper thread of the scene update.
// Header-only on include/henjou_hip.h and the standard library, as render_job.hpp is.  None of the three calls the library: they take
// callables, so tests/native/frame_loop_test.cpp drives them with fakes, without a GPU and under the sanitizers.
#pragma once
#include <condition_variable>
#include <cstring>
#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/henjou_hip.h"

namespace hjr {

// ---- the sample passes of one frame
struct PassRun {
    int rc = HJR_OK;          // the first failure of launch, after_pass or adaptive_state; nothing is called after it
    uint32_t done = 0;        // launches that succeeded
    bool queried = false;     // adaptive_state was asked at least once: `state` is its last answer, else it is zero
    bool stopped = false;     // ... and that answer was "no tile active": the frame ended with that pass (the last one included)
    hjr_adaptive_state state;
};

// Renders the frame of `p` in the passes that end at `ends` (pass_ends, render_job.hpp); `split` says that the job asked for more than one
// pass ("passes" > 1).  Per pass, in this order: launch(p); after_pass(k), k the passes done so far; adaptive_state(state), and the frame
// ends when it reports no active tile.  The two hooks may be empty.  The one behaviour where the three loops this replaces differed:
//   * p.sample_begin / sample_end are set only when the frame really has more than one pass (split, and more than one end).  A frame that
//     comes out as a single pass although the job asked for several (one chunk) is launched as the whole frame, [0, 0): the render calls
//     read [0, spp) as exactly that (check_pass, csrc/hjr_render.hip), so the copy that sent [0, spp) made the same launch;
//   * the adaptive query runs only behind such a pass, never behind a whole-frame launch (which has no adaptive state);
//   * a pass that ends where the previous one ended is skipped.  pass_ends gives none for spp > 0.  The first pass is never skipped: it
//     is empty only for spp == 0, and that frame goes to the render call, which refuses it.
inline PassRun render_passes(const std::vector<uint32_t>& ends, hjr_params& p, bool split, const std::function<int(hjr_params&)>& launch,
                             const std::function<int(uint32_t)>& after_pass = nullptr, const std::function<int(hjr_adaptive_state&)>& adaptive_state = nullptr)
{
    PassRun r;
    HJR_INIT(r.state);
    const bool several = split && ends.size() > 1;
    uint32_t begin = 0;
    for (size_t k = 0; k < ends.size(); k++) {
        const uint32_t end = ends[k];
        if (k && end <= begin) continue;
        if (several) { p.sample_begin = begin; p.sample_end = end; }
        if ((r.rc = launch(p)) != HJR_OK) return r;
        begin = end;
        r.done++;
        if (after_pass && (r.rc = after_pass(r.done)) != HJR_OK) return r;
        if (several && adaptive_state) {
            if ((r.rc = adaptive_state(r.state)) != HJR_OK) return r;
            r.queried = true;
            r.stopped = r.state.active_tiles == 0;
            if (r.stopped) return r;
        }
    }
    return r;
}

// ---- the output stage: two frame buffers in rotation, the sink (float4 -> sRGB8 -> PNG -> file) on a writer thread, so the producer
// renders frame f + 1 while frame f is written.  One producer thread.  Per frame: acquire, fill the buffer, submit; after the last frame
// drain.  The sink sees the frames in submission order, at most two are outstanding, and a slot is not handed out again before the sink has
// returned from it.  The first sink error wins: it is kept, code and text, and given to the producer once, by whichever of acquire, submit
// and drain comes next; frames submitted after it still go to the sink and their errors are dropped.  `serial`: no thread, submit runs the
// sink before it returns, everything else is the same.  After drain the writer is serial.  The destructor lets the sink finish the
// submitted frames and joins, so an exception that unwinds the producer does not end the program.
class FrameWriter {
public:
    using Sink = std::function<int(const float* rgba, const std::string& name, std::string& err)>;
    FrameWriter(size_t floats_per_frame, Sink sink, bool serial) : sink_(std::move(sink))
    {
        for (Slot& s : slots_) s.color.resize(floats_per_frame);
        if (!serial) thread_ = std::thread([this] { run(); });
    }
    FrameWriter(const FrameWriter&) = delete;
    FrameWriter& operator=(const FrameWriter&) = delete;
    ~FrameWriter() { stop(); }

    // the buffer of the next frame in `buf`; waits while the writer still has that slot (the frame two back)
    int acquire(float*& buf, std::string& err)
    {
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [&] { return !slots_[cur_].full; });
        buf = slots_[cur_].color.data();
        return report(err);
    }
    // hands the acquired buffer over, to be written as `name`
    int submit(const std::string& name, std::string& err)
    {
        Slot& s = slots_[cur_];
        s.name = name;
        if (thread_.joinable()) {
            { std::lock_guard<std::mutex> lk(mu_); s.full = true; }
            cv_.notify_all();
            cur_ ^= 1;
        } else consume(s);
        std::lock_guard<std::mutex> lk(mu_);
        return report(err);
    }
    // waits until every submitted frame has been through the sink and ends the thread
    int drain(std::string& err)
    {
        stop();
        std::lock_guard<std::mutex> lk(mu_);
        return report(err);
    }

private:
    struct Slot { std::vector<float> color; std::string name; bool full = false; };
    int report(std::string& err) // (mu_ held)
    {
        if (rc_ == HJR_OK || told_) return HJR_OK;
        told_ = true;
        err = err_;
        return rc_;
    }
    void consume(Slot& s)
    {
        std::string e;
        const int r = sink_(s.color.data(), s.name, e);
        std::lock_guard<std::mutex> lk(mu_);
        s.full = false;
        if (r != HJR_OK && rc_ == HJR_OK) { rc_ = r; err_ = e; }
    }
    void run() // the slots in rotation, as the producer fills them; quits only with nothing pending
    {
        for (int next = 0;; next ^= 1) {
            {
                std::unique_lock<std::mutex> lk(mu_);
                cv_.wait(lk, [&] { return slots_[next].full || quit_; });
                if (!slots_[next].full) return;
            }
            consume(slots_[next]);
            cv_.notify_all();
        }
    }
    void stop()
    {
        if (!thread_.joinable()) return;
        { std::lock_guard<std::mutex> lk(mu_); quit_ = true; }
        cv_.notify_all();
        thread_.join();
    }

    Sink sink_;
    Slot slots_[2];
    int cur_ = 0; // the producer's slot
    std::mutex mu_; // guards full, quit_, rc_, err_, told_
    std::condition_variable cv_;
    bool quit_ = false, told_ = false;
    int rc_ = HJR_OK;
    std::string err_;
    std::thread thread_;
};

// ---- the scene update of frame f + 1 (host: TRS evaluation, flatten, BVH build) on a helper thread while frame f renders.  start(frame)
// runs prepare(frame) there; take() joins and gives its result, and for a failure the text last_error() returned ON THAT THREAD (the
// library's hjr_last_error() is thread-local, so the caller's thread would not see it).  `serial`: start runs both on the caller's thread.
// One update at a time: start behind a result that was not taken is refused with HJR_ERR_STATE and starts nothing.  take() with nothing
// started is HJR_OK.  The destructor joins.
// THE RULE FOR THE CALLER: whatever must not run concurrently with prepare -- the drivers' hjr_set_morph_weights against
// hjr_prepare_transforms -- is called on the caller's own thread after take() has returned and before the next start().
class ScenePrefetch {
public:
    ScenePrefetch(std::function<int(uint32_t)> prepare, std::function<std::string()> last_error, bool serial)
        : prepare_(std::move(prepare)), last_error_(std::move(last_error)), serial_(serial) {}
    ScenePrefetch(const ScenePrefetch&) = delete;
    ScenePrefetch& operator=(const ScenePrefetch&) = delete;
    ~ScenePrefetch() { if (thread_.joinable()) thread_.join(); }

    int start(uint32_t frame)
    {
        if (pending_) return HJR_ERR_STATE;
        pending_ = true;
        auto work = [this, frame] {
            rc_ = prepare_(frame);
            if (rc_ != HJR_OK) err_ = last_error_();
        };
        if (serial_) work();
        else thread_ = std::thread(work);
        return HJR_OK;
    }
    int take(std::string& err)
    {
        if (thread_.joinable()) thread_.join();
        if (!pending_) return HJR_OK;
        pending_ = false;
        if (rc_ != HJR_OK) err = err_;
        return rc_;
    }

private:
    std::function<int(uint32_t)> prepare_;
    std::function<std::string()> last_error_;
    const bool serial_;
    bool pending_ = false; // (the caller's thread only)
    int rc_ = HJR_OK;      // written by the update, read after the join
    std::string err_;
    std::thread thread_;
};

} // namespace hjr
