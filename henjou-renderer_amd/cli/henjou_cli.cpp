// henjou_cli <render_option.json> [device] [--devices N]
// Stands in for the reference's missing main() (HenjouRenderer/henjouRenderer.cpp: Renderer r; r.initializeAndRender(path)).
//
// One GPU: hjr_render_file.  N GPUs of one node ("Henjou_HIP": {"devices": N} in the JSON, or --devices N): this process forks N
// rank processes BEFORE anything touches a GPU (fork + exec of itself with --rank), one per GPU; each loads the scene, renders its
// 8x8 pixel tiles of every frame (tile t -> rank t % N, HJR_FLAG_PACKED: only owned tiles are produced, [owned tile][64] float4)
// and the ranks meet in ONE RCCL collective per frame: ncclGather of the packed tiles onto rank 0 over xGMI (point-to-point sends,
// all peers in parallel, 1 / N of the frame per rank; SURVEY.md §8e option b).  Rank 0 scatters the N blocks into the frame
// (hjr_unpack_tiles_device), downloads it and writes <image_name>_<fff>.png exactly like the single-GPU path.  The assembled
// frame is bit-identical to the 1-GPU frame: per-pixel sample order does not depend on which GPU owns the pixel.
// Render_mode Denoise / DenoiseUpScale2X: the ranks render the guide AOVs (and the variance AOV) too, the gather moves them in the same one
// collective, and rank 0 runs hjr_denoise_shards_device: assemble, temporal accumulation, filter, upscale (DESIGN.md §7 "Denoise modes").
// The RCCL id travels over pipes the ranks inherit from the launcher (rank 0 -> launcher -> every other rank): no file, no name
// another user of the machine could guess.  A rank does everything that can fail (config, scene, device context, uploads) BEFORE it
// joins the communicator; the launcher reaps its children as they end, and the first one that fails or is signalled makes it
// terminate the others (SIGTERM, then SIGKILL), which may already be blocked inside ncclCommInitRank / ncclGather: a bad
// --devices value or a bad asset ends the job with exit code 1 instead of hanging it with the GPUs held.
// The reference has no counterpart (one process, one stream: renderer/renderer.h:1077-1078).
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>
#include <poll.h>
#include <signal.h>
#include <sys/wait.h>
#include <unistd.h>

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../host/frame_loop.hpp"
#include "../host/render_job.hpp"

#define HIPX(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { fprintf(stderr, "henjou_cli[%d]: %s: %s\n", rank, #call, hipGetErrorString(e_)); return 1; } } while (0)
#define NCCLX(call) do { ncclResult_t e_ = (call); if (e_ != ncclSuccess) { fprintf(stderr, "henjou_cli[%d]: %s: %s\n", rank, #call, ncclGetErrorString(e_)); return 1; } } while (0)
#define HJRX(call) do { int e_ = (call); if (e_ != HJR_OK) { fprintf(stderr, "henjou_cli[%d]: %s -> %d: %s\n", rank, #call, e_, hjr_last_error()); return 1; } } while (0)

// reads / writes exactly n bytes (false on EOF or error)
static bool io_all(int fd, void* buf, size_t n, bool write_it)
{
    char* b = (char*)buf;
    while (n) {
        const ssize_t k = write_it ? write(fd, b, n) : read(fd, b, n);
        if (k <= 0) return false;
        b += k; n -= (size_t)k;
    }
    return true;
}

// one rank of a multi-GPU render (its own process; GPU `rank` of the node)
static int run_rank(const char* json, int rank, int world, int id_fd)
{
    hjr::RenderOptionW opt; // (the long form: "window" and "bucket" behind hjr_render_option)
    memset(static_cast<void*>(&opt), 0, sizeof(opt));
    opt.struct_size = (uint32_t)sizeof(opt);
    HJRX(hjr_load_render_option_window(json, &opt));
    // Denoise modes (DESIGN.md §7 "Denoise modes"): every rank renders its tiles with the guide AOVs, and the variance AOV when the filter
    // options ask for it, into ONE per-rank buffer colour | albedo | normal | variance; the frame's one gather moves that buffer, and rank 0
    // assembles, accumulates and filters (hjr_denoise_shards_device).  The filter needs the whole frame, so it is not distributed.
    // The refusals and the sizes are hjr_render_file's (host/render_job.hpp); "firefly_clamp" is per pixel, so every rank clamps its own
    hjr::Job job;
    std::string refusal;
    if (!hjr::job_check(opt, job, refusal)) { fprintf(stderr, "henjou_cli: %s\n", refusal.c_str()); return 1; }
    if (world > 1 && hjr::multi_gpu_refusal(opt, refusal)) { fprintf(stderr, "henjou_cli: %s\n", refusal.c_str()); return 1; }
    const bool denoise = job.denoise, with_var = job.with_var;
    const uint32_t W = job.w, H = job.h, OW = job.out_w, OH = job.out_h; // the render size; the PNG's size
    hjr_scene* scene = nullptr;
    HJRX(hjr_scene_load_gltf(opt.gltf_path, opt.gltf_name, &opt, &scene));
    hjr_scene_view view;
    HJR_INIT(view);
    HJRX(hjr_scene_get_view(scene, &view));
    hjr_ctx* ctx = nullptr;
    HJRX(hjr_create(rank, &ctx));
    // every rank builds and renders; rank 0 also filters, accumulates and upscales, and has the frame data for it: it renders its own tiles
    HJRX(hjr::for_each_option(opt, hjr::rank_of_world(rank), [&](const char* key, int value) { return hjr_set_option(ctx, key, value); }));
    HJRX(hjr_upload_scene(ctx, &view));
    // "noise_threshold": each rank stops its own converged tiles between the sample passes (the rule does not depend on the rank); the one
    // gather per frame is unchanged.  A rank without tiles has nothing to adapt.
    const bool adaptive = job.adaptive && hjr_owned_tiles(W, H, (uint32_t)rank, (uint32_t)world) > 0;
    if (adaptive) HJRX(hjr::set_adaptive(ctx, opt));
    HJRX(hjr::upload_assets(ctx, opt, view, rank == 0));
    std::vector<float> morph_w; // "morph_targets": every rank blends the whole scene, so the PNGs are the single-GPU bytes
    HJRX(hjr::set_morph(ctx, opt, scene, morph_w));
    // RCCL communicator: rank 0 creates the id and writes it to its pipe; the launcher passes it on to the pipes of the other ranks
    // (a world of one needs no hand-over).  Everything fallible that does not need the peers has happened above.
    HIPX(hipSetDevice(rank));
    ncclUniqueId id;
    if (rank == 0) {
        NCCLX(ncclGetUniqueId(&id));
        if (world > 1 && !io_all(id_fd, &id, sizeof(id), true)) { fprintf(stderr, "henjou_cli[0]: cannot hand the RCCL id to the launcher\n"); return 1; }
    } else if (!io_all(id_fd, &id, sizeof(id), false)) { fprintf(stderr, "henjou_cli[%d]: no RCCL id from rank 0\n", rank); return 1; }
    if (id_fd >= 0) close(id_fd);
    ncclComm_t comm;
    NCCLX(ncclCommInitRank(&comm, world, id, rank));
    hipStream_t st;
    HIPX(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));

    const size_t block = (size_t)hjr_owned_tiles(W, H, 0, (uint32_t)world) * 64; // slots per rank and AOV (rank 0 owns the most tiles; others pad)
    const size_t rank_floats = block * (denoise ? (with_var ? 13u : 12u) : 4u);  // the per-rank buffer: three float4 AOVs and one float, or the colour alone
    float *d_packed = nullptr, *d_all = nullptr, *d_frame = nullptr;
    HIPX(hipMalloc(&d_packed, rank_floats * 4));
    HIPX(hipMemset(d_packed, 0, rank_floats * 4));
    float *const d_albedo = denoise ? d_packed + block * 4 : nullptr, *const d_normal = denoise ? d_packed + block * 8 : nullptr;
    float* const d_var = with_var ? d_packed + block * 12 : nullptr;
    std::vector<float> frame;
    if (rank == 0) {
        HIPX(hipMalloc(&d_all, rank_floats * 4 * world));
        HIPX(hipMalloc(&d_frame, (size_t)OW * OH * 16));
        frame.resize((size_t)OW * OH * 4);
    }
    std::vector<float> m((size_t)view.n_instances * 12), inv((size_t)view.n_instances * 12);
    for (uint32_t f = opt.start_frame; f < opt.end_frame; f++) {
        const float time = f / float(opt.fps); // renderer.h:1128
        HJRX(hjr_scene_eval_transforms(scene, time, m.data(), inv.data()));
        HJRX(hjr::set_morph_weights(ctx, scene, time, morph_w));
        HJRX(hjr_set_transforms(ctx, m.data(), inv.data(), view.n_instances));
        hjr_params_window pw; // (the longer caller: the render window behind hjr_params)
        memset(&pw, 0, sizeof(pw));
        hjr_params& p = pw.p;
        HJRX(hjr::frame_params(opt, scene, f, job.frame_w, job.frame_h, p));
        p.struct_size = (uint32_t)sizeof(pw);
        if (job.win) memcpy(pw.window, opt.window, sizeof(pw.window)); // "window": W x H is the window's size; the ranks shard the window's tiles
        p.rank = (uint32_t)rank; p.world_size = (uint32_t)world; p.flags |= HJR_FLAG_PACKED;
        const auto t0 = std::chrono::steady_clock::now();
        // "passes": the frame in sample passes, split as hjr_render_file splits it; the last pass leaves the frame's tiles in d_packed
        // (no after_pass hook: a per-pass hjr_get_stats would wait for the device; a frame of a single pass is a whole-frame render, not adaptive)
        std::function<int(hjr_adaptive_state&)> adaptive_state;
        if (adaptive) adaptive_state = [ctx](hjr_adaptive_state& as) { return hjr_get_adaptive_state(ctx, &as); };
        hjr_params_window pass = pw; // (the passes' ranges go into this copy: `p` stays the whole frame, which rank 0 ends below)
        const hjr::PassRun run = hjr::render_passes(hjr::pass_ends(p.spp, opt.passes ? opt.passes : 1u), pass.p, opt.passes > 1, [&](hjr_params& q) {
            return hjr_render_device_var(ctx, &q, d_packed, d_albedo, d_normal, d_var, st); // (Default: the colour alone, hjr_render_device's launch)
        }, nullptr, adaptive_state);
        if (run.rc != HJR_OK) { fprintf(stderr, "henjou_cli[%d]: sample pass %u of frame %u -> %d: %s\n", rank, run.done + 1, f, run.rc, hjr_last_error()); return 1; }
        const uint32_t n_done = run.done;
        if (run.queried)
            fprintf(stderr, "[henjou %d/%d] frame %u: adaptive: %u of %u tiles active at %u spp, %llu samples rendered\n", rank, world, f, run.state.active_tiles,
                    run.state.owned_tiles, run.state.sample_end, (unsigned long long)run.state.samples_rendered);
        NCCLX(ncclGather(d_packed, d_all, rank_floats, ncclFloat, 0, comm, st)); // the one data-path collective of a frame
        if (rank == 0 && denoise) { // the gathered blocks -> frames -> (temporal accumulation) -> filter -> (upscale), all on st
            hjr_shards sh;
            HJR_INIT(sh);
            sh.world_size = (uint32_t)world; sh.rank_stride = rank_floats * 4;
            sh.color = d_all; sh.albedo = d_all + block * 4; sh.normal = d_all + block * 8;
            sh.variance = with_var ? d_all + block * 12 : nullptr;
            hjr_params whole = p; // the gather follows the frame's last pass: rank 0 ends the frame (the history advances once per frame)
            whole.struct_size = (uint32_t)sizeof(whole); // (a plain hjr_params: the Denoise modes take no window)
            HJRX(hjr_denoise_shards_device(ctx, &whole, opt.render_mode, &sh, d_frame, OW, OH, st));
            HIPX(hipMemcpyAsync(frame.data(), d_frame, frame.size() * 4, hipMemcpyDeviceToHost, st));
        } else if (rank == 0) {
            for (int r = 0; r < world; r++) HJRX(hjr_unpack_tiles_device(ctx, d_all + (size_t)r * block * 4, W, H, (uint32_t)r, (uint32_t)world, d_frame, st));
            HIPX(hipMemcpyAsync(frame.data(), d_frame, frame.size() * 4, hipMemcpyDeviceToHost, st));
        }
        HIPX(hipStreamSynchronize(st));
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        hjr_stats s;
        HJR_INIT(s);
        if (hjr_get_stats(ctx, &s) == HJR_OK)
            fprintf(stderr, "[henjou %d/%d] frame %u: kernel %.3f ms, render + gather + assemble %.3f ms%s\n", rank, world, f, s.last_kernel_ms, ms,
                    n_done > 1 ? (", " + std::to_string(n_done) + " sample passes").c_str() : "");
        if (rank == 0) {
            std::vector<uint8_t> rgba8((size_t)OW * OH * 4);
            HJRX(hjr_float4_to_srgb8(frame.data(), rgba8.data(), OW * OH));
            HJRX(hjr_write_png(hjr::frame_png_name(opt, f).c_str(), rgba8.data(), OW, OH, 1));
        }
    }
    ncclCommDestroy(comm);
    hjr_destroy(ctx);
    hjr_scene_free(scene);
    return 0;
}

int main(int argc, char** argv)
{
    const char* path = "render_option.json";
    int device = 0, devices = 0, rank = -1, world = 0, id_fd = -1;
    int positional = 0;
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        if (a == "--devices" && i + 1 < argc) devices = atoi(argv[++i]);
        else if (a == "--rank" && i + 1 < argc) rank = atoi(argv[++i]);
        else if (a == "--world" && i + 1 < argc) world = atoi(argv[++i]);
        else if (a == "--id-fd" && i + 1 < argc) id_fd = atoi(argv[++i]);
        else if (positional == 0) { path = argv[i]; positional++; }
        else if (positional == 1) { device = atoi(argv[i]); positional++; }
    }
    // a rank process of a multi-GPU render (world 1: the same code path on one GPU, no id hand-over)
    if (rank >= 0) return (world >= 1 && rank < world && (world == 1 || id_fd >= 0)) ? run_rank(path, rank, world, id_fd) : 2;
    hjr::RenderOptionW opt;
    memset(static_cast<void*>(&opt), 0, sizeof(opt));
    opt.struct_size = (uint32_t)sizeof(opt);
    const bool parsed = hjr_load_render_option_window(path, &opt) == HJR_OK; // (host-only parse: no GPU is touched here)
    if (devices == 0) { // the JSON decides
        if (!parsed) { fprintf(stderr, "henjou_cli: error: %s\n", hjr_last_error()); return 1; }
        devices = (int)opt.devices;
    }
    std::string refusal; // what no world of several ranks renders: said once, before a rank is started (a file that does not parse is the ranks' to report)
    if (devices > 1 && parsed && hjr::multi_gpu_refusal(opt, refusal)) { fprintf(stderr, "henjou_cli: %s\n", refusal.c_str()); return 1; }
    if (devices <= 1) {
        int rc = hjr_render_file(path, device);
        if (rc != HJR_OK) { fprintf(stderr, "henjou_cli: error %d: %s\n", rc, hjr_last_error()); return 1; }
        return 0;
    }
    // launcher: one rank process per GPU, started before any GPU call in this process.  Pipes: up[0] <- rank 0 (the id), down[r] -> rank r.
    signal(SIGPIPE, SIG_IGN); // a rank that died before reading its id must not take the launcher down
    int up[2] = { -1, -1 };
    if (pipe(up) != 0) { perror("henjou_cli: pipe"); return 1; }
    std::vector<int> down((size_t)devices, -1);
    std::vector<pid_t> kids;
    auto kill_all = [&]() {
        for (pid_t k : kids) if (k > 0) kill(k, SIGTERM);
        for (int t = 0; t < 50; t++) { // 5 s of grace, then SIGKILL
            bool any = false;
            for (pid_t& k : kids) if (k > 0) { int stt; if (waitpid(k, &stt, WNOHANG) == k) k = -1; else any = true; }
            if (!any) return;
            std::this_thread::sleep_for(std::chrono::milliseconds(100));
        }
        for (pid_t& k : kids) if (k > 0) { kill(k, SIGKILL); int stt; waitpid(k, &stt, 0); k = -1; }
    };
    for (int r = 0; r < devices; r++) {
        int pd[2] = { -1, -1 };
        if (r > 0 && pipe(pd) != 0) { perror("henjou_cli: pipe"); kill_all(); return 1; }
        const pid_t pid = fork();
        if (pid < 0) { perror("henjou_cli: fork"); kill_all(); return 1; }
        if (pid == 0) {
            // the child keeps exactly one pipe end: rank 0 the write end of `up`, rank r the read end of its own `down` pipe
            close(up[0]);
            for (int q = 1; q < r; q++) if (down[(size_t)q] >= 0) close(down[(size_t)q]);
            int mine = up[1];
            if (r > 0) { close(up[1]); close(pd[1]); mine = pd[0]; }
            const std::string rs = std::to_string(r), ws = std::to_string(devices), fs = std::to_string(mine);
            execl("/proc/self/exe", argv[0], path, "--rank", rs.c_str(), "--world", ws.c_str(), "--id-fd", fs.c_str(), (char*)nullptr);
            perror("henjou_cli: exec");
            _exit(127);
        }
        kids.push_back(pid);
        if (r > 0) { close(pd[0]); down[(size_t)r] = pd[1]; }
    }
    close(up[1]);
    // wait for rank 0's id and for children at the same time: the first child that fails ends the job
    int rc = 0, alive = devices;
    bool id_sent = false;
    ncclUniqueId id;
    size_t got = 0;
    while (alive > 0 && rc == 0) {
        if (!id_sent) {
            struct pollfd pf = { up[0], POLLIN, 0 };
            if (poll(&pf, 1, 100) > 0) {
                const ssize_t k = read(up[0], (char*)&id + got, sizeof(id) - got);
                if (k > 0) got += (size_t)k;
                else if (k == 0 && got < sizeof(id)) { /* rank 0 closed its end without an id: its exit status follows */ std::this_thread::sleep_for(std::chrono::milliseconds(50)); }
                if (got == sizeof(id)) {
                    for (int r = 1; r < devices; r++) { (void)io_all(down[(size_t)r], &id, sizeof(id), true); close(down[(size_t)r]); down[(size_t)r] = -1; } // (a dead reader shows up as a failed child below)
                    id_sent = true;
                }
            }
        } else std::this_thread::sleep_for(std::chrono::milliseconds(50));
        for (;;) {
            int stt = 0;
            const pid_t k = waitpid(-1, &stt, WNOHANG);
            if (k <= 0) break;
            for (pid_t& q : kids) if (q == k) { q = -1; alive--; }
            if (!WIFEXITED(stt) || WEXITSTATUS(stt) != 0) {
                fprintf(stderr, "henjou_cli: a rank process %s; stopping the others\n", WIFEXITED(stt) ? "failed" : "was killed by a signal");
                rc = 1;
            }
        }
    }
    if (rc != 0) kill_all();
    close(up[0]);
    for (int fd : down) if (fd >= 0) close(fd);
    return rc;
}
