// Device context of libhenjou_hip.so: HBM-resident scene, per-frame BVH upload, kernel launch and timing.
// Replaces the reference's CUDA/OptiX plumbing (renderer/renderer.h:197-255 upload, 293-739 context/GAS/IAS/pipeline/SBT,
// 1175-1242 Params fill + optixLaunch).  No CPU fallback exists: without a gfx950 device every entry point fails loudly.
// This unit: the context's lifetime, options, scene and transform uploads, statistics; hjr_render.hip, hjr_post.hip and hjr_util.hip hold the rest.
#include <chrono>
#include "hjr_device_internal.h"
#ifdef HJR_UNITY /* diagnostic variants (make variant): one translation unit, so that the __device__ diagnostic counters are one symbol */
#include "hjr_launch.hip.h"
#endif

extern "C" int hjr_create(int device, hjr_ctx** out)
{
    if (!out) { set_error("hjr_create: null out pointer"); return HJR_ERR_ARG; }
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        set_error(std::string("hjr_create: no HIP device available (") + hipGetErrorString(e) + "); this library has no CPU fallback");
        return HJR_ERR_DEVICE;
    }
    if (device < 0 || device >= n) { set_error("hjr_create: device ordinal out of range"); return HJR_ERR_ARG; }
    HIPCHK(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        set_error(std::string("hjr_create: device is ") + prop.gcnArchName + ", this library carries gfx950 (MI355X) code objects only");
        return HJR_ERR_DEVICE;
    }
    hjr_ctx* c = new hjr_ctx();
    c->device = device;
    c->n_cus = prop.multiProcessorCount;
    memset(&c->stats, 0, sizeof(c->stats));
#ifdef HJR_ENV_OPTIONS /* experiment builds only (make variant): every option also from the environment, HJR_<KEY> */
    for (int i = 0; i < hjr::OPT_COUNT; i++) {
        std::string name = std::string("HJR_") + hjr::opt_table()[i].key;
        for (char& ch : name) ch = (char)toupper((unsigned char)ch);
        if (const char* e = getenv(name.c_str())) { const int v = atoi(e); if (v >= hjr::opt_table()[i].lo && v <= hjr::opt_table()[i].hi) c->opt.v[i] = v; }
    }
    if (c->opt.is_set(hjr::OPT_HOST_THREADS)) hjr::set_host_threads(c->opt.v[hjr::OPT_HOST_THREADS]);
#endif
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess || hipEventCreate(&c->ev0) != hipSuccess ||
        hipEventCreate(&c->ev1) != hipSuccess) {
        set_error("hjr_create: stream/event creation failed");
        delete c;
        return HJR_ERR_DEVICE;
    }
    *out = c;
    return HJR_OK;
}

// Tuning / test options (host/options.hpp lists keys, ranges and defaults; include/henjou_hip.h documents them)
extern "C" int hjr_set_option(hjr_ctx* c, const char* key, int value)
{
    if (!c) { set_error("hjr_set_option: null context"); return HJR_ERR_ARG; }
    const int i = hjr::opt_find(key);
    if (i < 0) { set_error(std::string("hjr_set_option: unknown option \"") + (key ? key : "(null)") + "\""); return HJR_ERR_ARG; }
    const hjr::OptDesc& d = hjr::opt_table()[i];
    if (value != -1 && (value < d.lo || value > d.hi || hjr::opt_hole(i, value))) {
        set_error(std::string("hjr_set_option: value out of range for \"") + d.key + "\" (" + std::to_string(d.lo) + " .. " + std::to_string(d.hi) + ", or -1 for the default)");
        return HJR_ERR_ARG;
    }
    c->opt.v[i] = value;
    // rule 10 keeps chunk sums from a frame's first pass on: an unfinished progressive frame cannot change its rule half way (as hjr_set_adaptive).
    // "firefly_clamp" alone with "firefly_clamp_passes" off keeps what it always did: the next pass is refused by check_pass
    if (i == hjr::OPT_FIREFLY_CLAMP_PASSES || (i == hjr::OPT_FIREFLY_CLAMP && c->opt.get(hjr::OPT_FIREFLY_CLAMP_PASSES, 0) == 1)) { c->pass.active = false; c->ad.frame = false; }
    if (i == hjr::OPT_ADAPTIVE_TEMPORAL) { c->pass.active = false; c->ad.frame = false; c->tmp.have_prior = false; } // rule 11: an unfinished progressive frame cannot change its rule half way (as hjr_set_adaptive); the history stays
    if (i == hjr::OPT_DENOISE_TEMPORAL || i == hjr::OPT_DENOISE_VARIANCE_SPATIAL || i == hjr::OPT_DENOISE_TEMPORAL_COVERAGE || i == hjr::OPT_DENOISE_TEMPORAL_MOMENTS || i == hjr::OPT_DENOISE_TEMPORAL_RESPONSE) c->tmp.have_prev = false; // setting any of these options drops the history
    if (i == hjr::OPT_HOST_THREADS) hjr::set_host_threads(value);
    return HJR_OK;
}
extern "C" int hjr_get_option(hjr_ctx* c, const char* key, int* value)
{
    if (!c || !value) { set_error("hjr_get_option: null argument"); return HJR_ERR_ARG; }
    const int i = hjr::opt_find(key);
    if (i < 0) { set_error(std::string("hjr_get_option: unknown option \"") + (key ? key : "(null)") + "\""); return HJR_ERR_ARG; }
    *value = c->opt.v[i];
    return HJR_OK;
}

extern "C" void hjr_destroy(hjr_ctx* c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();
    if (c->ad.h_active) (void)hipHostFree(c->ad.h_active);
    if (c->ad.ready) (void)hipEventDestroy(c->ad.ready);
    c->dbvh.release();
    c->deform.dev.drop();
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c; // every DevBuf of the context, with its device still current
}

extern "C" int hjr_upload_scene(hjr_ctx* c, const hjr_scene_view* v)
{
    if (!c || !v) { set_error("hjr_upload_scene: null argument"); return HJR_ERR_ARG; }
    hjr_scene_view view; // sized struct: only the bytes the caller owns are read
    if (!hjr::abi_take(v, view, "hjr_upload_scene")) return HJR_ERR_ARG;
    v = &view;
    std::string err;
    if (!c->scene.set(*v, err)) { set_error("hjr_upload_scene: " + err); return HJR_ERR_ARG; }
    HIPCHK(hipSetDevice(c->device));
    static_assert(sizeof(hjr_material) == HJR_MAT_F4 * 16, "hjr_material must be HJR_MAT_F4 x float4");
    if (!c->d_materials.upload(c->scene.materials.data(), c->scene.materials.size() * sizeof(hjr_material), c->stream)) {
        set_error("hjr_upload_scene: material upload failed");
        return HJR_ERR_DEVICE;
    }
    // textureBind (renderer.h:740-800): RGBA8 atlas + per-slot descriptors + the sRGB decode table
    c->n_textures = (uint32_t)c->scene.textures.size();
    if (c->n_textures) {
        std::vector<uint32_t> desc;
        for (auto& t : c->scene.textures) { desc.push_back(t.offset); desc.push_back(t.width); desc.push_back(t.height); desc.push_back((uint32_t)t.srgb); }
        float lut[256];
        for (int i = 0; i < 256; i++) {
            double v = (double)i / 255.0;
            lut[i] = (float)(v <= 0.04045 ? v / 12.92 : pow((v + 0.055) / 1.055, 2.4));
        }
        if (!c->d_texels.upload(c->scene.texels.data(), c->scene.texels.size() * 4, c->stream) ||
            !c->d_tex_desc.upload(desc.data(), desc.size() * 4, c->stream) || !c->d_srgb_lut.upload(lut, sizeof(lut), c->stream)) {
            set_error("hjr_upload_scene: texture upload failed");
            return HJR_ERR_DEVICE;
        }
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    c->frame_gen++;
    c->tmp.have_prev = false; // temporal history: another scene
    c->have_scene = true;
    c->have_frame = false;
    c->dbvh.have_scene = false; // the device builder uploads the new scene at its next build
    c->dbvh.topo.valid = false; // ... and "device_bvh_instances" builds its topology again
    c->refit = hjr_ctx::Refit(); // ... which is a full one
    c->deform.morph = hjr::Morph(); // the morph belonged to the scene before
    c->deform.dev.drop();
    c->deform.vert = std::vector<float>(); c->deform.norm = std::vector<float>();
    c->deform.gen++;
    return HJR_OK;
}

// ---- deforming meshes (include/henjou_hip.h) ----
// what the three calls share once their arguments are accepted: the geometry is another one
static void geometry_changed(hjr_ctx* c)
{
    c->deform.gen++;            // the next prepare is not "unchanged"
    c->frame_gen++;             // an unfinished progressive frame ends (as hjr_set_sky)
    c->tmp.have_prev = false;   // temporal history: reprojection is rigid per instance and cannot follow a deforming surface
    c->dbvh.topo.valid = false; // "device_bvh_instances": the topology is built again at the next commit
}

extern "C" int hjr_update_vertices(hjr_ctx* c, uint32_t first_vertex, uint32_t n_vertices, const float* positions, const float* normals)
{
    if (!c) { set_error("hjr_update_vertices: null context"); return HJR_ERR_ARG; }
    if (!c->have_scene) { set_error("hjr_update_vertices: no scene uploaded"); return HJR_ERR_STATE; }
    if (!positions) { set_error("hjr_update_vertices: null positions"); return HJR_ERR_ARG; }
    const size_t nv = c->scene.vertices.size() / 3;
    if (n_vertices == 0 || (uint64_t)first_vertex + n_vertices > nv) { set_error("hjr_update_vertices: vertex range outside the scene"); return HJR_ERR_ARG; }
    const size_t off = 3 * (size_t)first_vertex, bytes = 12 * (size_t)n_vertices;
    if (c->dbvh.have_scene) { // the device builder's copy of the base; nothing a render reads
        HIPCHK(hipSetDevice(c->device));
        HIPCHK(hipMemcpyAsync(c->dbvh.vert.as<float>() + off, positions, bytes, hipMemcpyHostToDevice, c->stream));
        if (normals) HIPCHK(hipMemcpyAsync(c->dbvh.norm.as<float>() + off, normals, bytes, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream)); // the caller's arrays are free on return
    }
    memcpy(&c->scene.vertices[off], positions, bytes);
    if (normals) memcpy(&c->scene.normals[off], normals, bytes);
    c->deform.dev.copied = false; // the working arrays of a morph: from the new base
    geometry_changed(c);
    return HJR_OK;
}

extern "C" int hjr_set_morph(hjr_ctx* c, const hjr_morph* m)
{
    if (!c) { set_error("hjr_set_morph: null context"); return HJR_ERR_ARG; }
    if (!c->have_scene) { set_error("hjr_set_morph: no scene uploaded"); return HJR_ERR_STATE; }
    hjr_morph mm;
    if (m) { if (!hjr::abi_take(m, mm, "hjr_set_morph")) return HJR_ERR_ARG; }
    else { memset(&mm, 0, sizeof(mm)); }
    std::string err;
    if (!c->deform.morph.set(mm, (uint32_t)(c->scene.vertices.size() / 3), err)) { set_error("hjr_set_morph: " + err); return HJR_ERR_ARG; }
    HIPCHK(hipSetDevice(c->device));
    c->deform.dev.drop(); // deltas, table and working arrays: uploaded at the next device build (none without a morph)
    if (!c->deform.morph.active()) { c->deform.vert = std::vector<float>(); c->deform.norm = std::vector<float>(); }
    geometry_changed(c);
    return HJR_OK;
}

extern "C" int hjr_set_morph_weights(hjr_ctx* c, const float* w, uint32_t n)
{
    if (!c) { set_error("hjr_set_morph_weights: null context"); return HJR_ERR_ARG; }
    hjr::Morph& mo = c->deform.morph;
    if (!mo.active()) { set_error("hjr_set_morph_weights: no morph set"); return HJR_ERR_STATE; }
    if (n != mo.weights.size()) { set_error("hjr_set_morph_weights: weight count does not match the morph's n_weights"); return HJR_ERR_ARG; }
    if (n && !w) { set_error("hjr_set_morph_weights: null weights"); return HJR_ERR_ARG; }
    const bool equal = n == 0 || memcmp(mo.weights.data(), w, (size_t)n * 4) == 0;
    if (n) memcpy(mo.weights.data(), w, (size_t)n * 4);
    if (equal) { c->frame_gen++; c->tmp.have_prev = false; } // the same bits: the same geometry, so frame data and topology built from it stay current
    else geometry_changed(c);
    return HJR_OK;
}

// updateIASMatrix + buildIAS (renderer.h:257-291, 398-490) in two halves, so that a frame loop can prepare frame f + 1 on the
// host (worker threads, no device access, no access to what a running render reads) while frame f renders:
//   hjr_prepare_transforms: flatten + BVH build into the context's prepared frame (hjr_ctx::prep);
//   hjr_commit_transforms:  upload the prepared data (after the previous render has finished) and make it current (hjr_ctx::built).
// hjr_set_transforms = prepare + commit.
extern "C" int hjr_prepare_transforms(hjr_ctx* c, const float* m, const float* inv, uint32_t n)
{
    if (!c || (n && (!m || !inv))) { set_error("hjr_set_transforms: null argument"); return HJR_ERR_ARG; }
    if (!c->have_scene) { set_error("hjr_set_transforms: no scene uploaded"); return HJR_ERR_STATE; }
    std::string err;
    hjr::BuildOptions bo; // options "lds_bvh", "lds_stack16", "bvh_width", "leaf_max", "verbose" (host build stages)
    bo.allow_lds = c->opt.get(hjr::OPT_LDS_BVH, 1) != 0;
    bo.prefer_stack16 = c->opt.get(hjr::OPT_LDS_STACK16, 0) != 0;
    bo.bvh_width = c->opt.get(hjr::OPT_BVH_WIDTH, -1);
    bo.leaf_max = c->opt.get(hjr::OPT_LEAF_MAX, -1);
    bo.refine = c->opt.get(hjr::OPT_BVH_REFINE, -1);
    bo.timing = c->opt.get(hjr::OPT_VERBOSE, 0) != 0;
    const bool device = c->opt.get(hjr::OPT_DEVICE_BVH, 0) != 0; // option "device_bvh": the build runs at hjr_commit_transforms
    if (device && (bo.bvh_width == 2 || c->opt.get(hjr::OPT_LDS_BVH, -1) == 1)) {
        set_error("hjr_set_transforms: \"device_bvh\" builds the BVH4 memory layout only; it cannot be combined with \"bvh_width\" 2 or \"lds_bvh\" 1");
        return HJR_ERR_ARG;
    }
    BuildKey key;
    key.allow_lds = bo.allow_lds; key.prefer_stack16 = bo.prefer_stack16; key.bvh_width = bo.bvh_width; key.leaf_max = bo.leaf_max; key.refine = bo.refine;
    key.device = device;
    key.opt_rounds = device ? (uint32_t)c->opt.get(hjr::OPT_DEVICE_BVH_OPT, 0) : 0u;
    key.instances = device && c->opt.get(hjr::OPT_DEVICE_BVH_INSTANCES, 0) != 0;
    key.graft = key.instances && c->opt.get(hjr::OPT_DEVICE_BVH_GRAFT, 0) != 0;
    hjr_ctx::Prepared& pp = c->prep;
    pp.valid = false;
    pp.same = false;
    // unchanged instance transforms (static geometry, e.g. a camera-only animation): the world-space arrays and the BVH of the
    // previous frame are still right; the reference re-uploads its IAS every frame (renderer.h:257-291), which costs it nothing
    const bool force_rebuild = c->opt.get(hjr::OPT_FORCE_REBUILD, 0) != 0; // benchmarking option
    hjr_ctx::Deform& df = c->deform;
    if (!force_rebuild && c->have_frame && df.built_gen == df.gen && c->built.key == key && c->built.m.size() == (size_t)n * 12 && n == c->scene.n_instances &&
        (n == 0 || (memcmp(c->built.m.data(), m, (size_t)n * 48) == 0 && memcmp(c->built.inv.data(), inv, (size_t)n * 48) == 0))) {
        pp.same = true;
        pp.valid = true;
        return HJR_OK;
    }
    const auto t_build0 = std::chrono::steady_clock::now();
    if (device) { // validation and the light table here; flatten + BVH at the commit, on the device
        if (n != c->scene.n_instances) { set_error("hjr_set_transforms: instance count does not match the uploaded scene"); return HJR_ERR_ARG; }
        pp.frame = hjr::FrameData();
        pp.frame.n_tris = c->scene.n_triangles;
        pp.frame.width = 4;
        pp.frame.lds_mode = 0;
        df.prep_w = df.morph.weights;
        hjr::build_lights(c->scene, m, inv, pp.frame, nullptr, nullptr, &df.morph, df.prep_w.data()); // a morph: only the light triangles' vertices are blended here
    } else {
        const bool morphed = df.morph.active(); // the working copy, on the worker threads; without a morph no copy and no pass
        if (morphed) hjr::morph_blend(c->scene, df.morph, df.morph.weights.data(), df.vert, df.norm);
        df.prep_vertices = morphed ? df.morph.n_vertices : 0u;
        if (!hjr::build_frame(c->scene, m, inv, n, bo, pp.frame, err, morphed ? df.vert.data() : nullptr, morphed ? df.norm.data() : nullptr)) {
            set_error("hjr_set_transforms: " + err);
            return HJR_ERR_ARG;
        }
    }
    df.prep_gen = df.gen;
    pp.build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_build0).count();
    pp.m.assign(m, m + (size_t)n * 12); pp.inv.assign(inv, inv + (size_t)n * 12); pp.key = key;
    pp.valid = true;
    return HJR_OK;
}

// option "device_bvh": the build of the prepared transforms as kernels on the context's stream, behind what is already queued there.
// It writes the builder's own buffers; they become current (swapped with d_nodes, d_tri_*, d_lights) only when it succeeds, so a
// failed build leaves the previous frame current.
// Option "device_bvh_refit": up to that many consecutive commits after a full build keep its topology and refit the boxes
// (hjr::device_bvh_refit), while the current data is a device build of this scene with these build options and the cost guard holds.
// `instances`: the instance subtrees the build made (0: an ordinary build or a refit), for hjr_stats and the verbose line.
static int commit_device(hjr_ctx* c, uint32_t& instances)
{
    const int leaf_max = c->opt.get(hjr::OPT_LEAF_MAX, (int)HJR_LEAF_DEFAULT);
    const int opt_rounds = c->opt.get(hjr::OPT_DEVICE_BVH_OPT, 0); // option "device_bvh_opt": treelet-restructuring rounds
    const uint32_t limit = (uint32_t)c->opt.get(hjr::OPT_DEVICE_BVH_REFIT, 0);
    hjr_ctx::Prepared& pp = c->prep;
    const uint32_t n_inst = (uint32_t)(pp.m.size() / 12), tag = pp.key.pack();
    hjr_ctx::Refit& rf = c->refit;
    // key.instances: per-instance trees kept in dbvh.topo, a top tree per commit; no refits with it
    // key.graft (only ever set with it): the instances' BVH4s collapsed once, grafted under a BVH4 top tree
    if (!pp.key.instances) c->dbvh.drop_topology();
    const bool refit = !pp.key.instances && c->have_frame && rf.device && c->dbvh.have_scene && !rf.rebuild && rf.count < limit && rf.tag == tag &&
                       c->built.m.size() == pp.m.size() && c->scene.n_triangles >= 2 && c->frame.n_tris == c->scene.n_triangles;
    hjr::DeviceBvhResult r;
    std::string err;
    hjr::FrameData& f = pp.frame;
    hjr::DeviceMorph* dm = &c->deform.dev; // hjr_set_morph: blended on the stream ahead of the flatten of whichever build runs
    dm->host = &c->deform.morph; dm->w_next = c->deform.morph.active() ? c->deform.prep_w.data() : nullptr; dm->launched = 0;
    const int rc = pp.key.instances ? hjr::device_bvh_instances(c->dbvh, c->scene, pp.m.data(), pp.inv.data(), n_inst, (uint32_t)leaf_max, (uint32_t)opt_rounds, tag, pp.key.graft,
                                                                f.lights.data(), f.lights.size(), c->stream, r, err, dm)
                   : refit ? hjr::device_bvh_refit(c->dbvh, c->scene, pp.m.data(), pp.inv.data(), n_inst, c->d_nodes, c->d_tri_geom, c->frame.n_nodes,
                                                 f.lights.data(), f.lights.size(), c->stream, r, err, dm)
                         : hjr::device_bvh_build(c->dbvh, c->scene, pp.m.data(), pp.inv.data(), n_inst, (uint32_t)leaf_max, (uint32_t)opt_rounds,
                                                 f.lights.data(), f.lights.size(), c->stream, r, err, dm);
    if (rc != HJR_OK) { set_error("hjr_set_transforms: " + err); return rc; }
    c->d_nodes.swap(c->dbvh.nodes); c->d_tri_geom.swap(c->dbvh.tri_geom); c->d_tri_shade.swap(c->dbvh.tri_shade);
    c->d_tri_inst.swap(c->dbvh.tri_inst); c->d_lights.swap(c->dbvh.lights);
    if (refit) { // the topology's
        f.n_nodes = c->frame.n_nodes; f.stack_need = c->frame.stack_need; f.depth = c->frame.depth;
        rf.count++;
        // the refit just made stays current; a tree that has grown past the guard is rebuilt at the next commit
        rf.rebuild = (double)r.sah > (double)rf.sah_full * (1.0 + c->opt.get(hjr::OPT_DEVICE_BVH_REFIT_GROWTH, 10) / 100.0);
    } else {
        f.n_nodes = r.n_nodes; f.stack_need = r.stack_need; f.depth = r.depth;
        rf.device = true; rf.rebuild = false; rf.count = 0; rf.tag = tag; rf.sah_full = r.sah;
    }
    rf.sah = r.sah;
    instances = r.instances;
    pp.build_ms = r.build_ms;
    return HJR_OK;
}

extern "C" int hjr_commit_transforms(hjr_ctx* c)
{
    if (!c) { set_error("hjr_commit_transforms: null context"); return HJR_ERR_ARG; }
    hjr_ctx::Prepared& pp = c->prep;
    if (!pp.valid) { set_error("hjr_commit_transforms: nothing prepared"); return HJR_ERR_STATE; }
    pp.valid = false;
    if (pp.same) {
        if (c->opt.get(hjr::OPT_VERBOSE, 0)) fprintf(stderr, "[hjr] transforms unchanged: frame data reused\n");
        c->stats.morph_vertices = 0; // nothing was blended for this commit
        return HJR_OK;
    }
    HIPCHK(hipSetDevice(c->device));
    c->frame_gen++; // the frame data is replaced (a progressive frame cannot continue on it, even if the build below fails)
    uint32_t instances = 0; // option "device_bvh_instances": instance subtrees of this commit (0: an ordinary build)
    if (pp.key.device) {
        if (const int rc = commit_device(c, instances)) return rc;
        std::swap(c->frame, pp.frame);
    } else {
        std::swap(c->frame, pp.frame);
        c->refit = hjr_ctx::Refit(); // host-built data: nothing to refit
        c->dbvh.drop_topology();
        const hjr::FrameData& f = c->frame;
        bool ok = c->d_nodes.upload(f.nodes.data(), f.nodes.size() * 4, c->stream) &&
                  c->d_tri_geom.upload(f.tri_geom.data(), f.tri_geom.size() * 4, c->stream) &&
                  c->d_tri_shade.upload(f.tri_shade.data(), f.tri_shade.size() * 4, c->stream) &&
                  c->d_tri_inst.upload(f.tri_inst.data(), f.tri_inst.size() * 4, c->stream) &&
                  c->d_lights.upload(f.lights.data(), f.lights.size() * 4, c->stream);
        if (!ok) { c->have_frame = false; set_error("hjr_set_transforms: device upload failed"); return HJR_ERR_DEVICE; }
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    const hjr::FrameData& f = c->frame;
    c->have_frame = true;
    c->built.m.swap(pp.m); c->built.inv.swap(pp.inv); c->built.key = pp.key;
    if (c->deform.built_gen != c->deform.prep_gen) c->tmp.have_prev = false; // the geometry takes effect here: a render since the call has made a history of the old one
    c->deform.built_gen = c->deform.prep_gen;
    c->stats.morph_vertices = pp.key.device ? c->deform.dev.launched : c->deform.prep_vertices;
    c->stats.geometry_generation = c->deform.built_gen;
    c->stats.bvh_nodes = f.n_nodes;
    c->stats.bvh_depth = f.depth;
    c->stats.bvh_builder = pp.key.device ? 1u : 0u;
    c->stats.frame_build_ms = (float)pp.build_ms;
    c->stats.bvh_refits = c->refit.count;
    c->stats.bvh_sah = c->refit.sah;
    c->stats.bvh_instances = instances;
    if (instances) c->stats.bvh_topology_ms = c->dbvh.topo.ms;
    const bool refitted = pp.key.device && c->refit.count > 0;
    if (c->opt.get(hjr::OPT_VERBOSE, 0))
        fprintf(stderr, "[hjr] BVH%u (lds_mode %d): %u nodes (%zu KB), %u triangles (%zu KB), stack %u entries/lane, %s %s %.1f ms\n", f.width, f.lds_mode, f.n_nodes,
                (size_t)f.n_nodes * (f.width == 2 ? HJR_NODE2_F4 : HJR_NODE4_F4) * 16 / 1024, f.n_tris, (size_t)std::max(f.n_tris, 1u) * HJR_TRI_F4 * 16 / 1024,
                f.stack_need, pp.key.device ? "device" : "host", refitted ? "refit" : (instances ? (pp.key.graft ? "grafted instance build" : "instance build") : "build"), pp.build_ms);
    if (c->opt.get(hjr::OPT_VERBOSE, 0) && c->stats.morph_vertices)
        fprintf(stderr, "[hjr] morph: %u vertices blended%s", c->stats.morph_vertices, pp.key.device ? "" : " on the host\n");
    if (c->opt.get(hjr::OPT_VERBOSE, 0) && c->stats.morph_vertices && pp.key.device) fprintf(stderr, " on the device, kernel %.4f ms\n", c->deform.dev.kernel_ms());
    c->stats.n_triangles = f.n_tris;
    return HJR_OK;
}

// inspection copy of the current frame data (tests): synchronous, from the device buffers the kernels read
extern "C" int hjr_copy_frame_data(hjr_ctx* c, int what, void* dst, size_t dst_bytes, size_t* bytes)
{
    if (!c || !bytes) { set_error("hjr_copy_frame_data: null argument"); return HJR_ERR_ARG; }
    if (!c->have_frame) { set_error("hjr_copy_frame_data: no frame data (set transforms first)"); return HJR_ERR_STATE; }
    const hjr::FrameData& f = c->frame;
    const DevBuf* src = nullptr;
    size_t n = 0;
    switch (what) {
    case HJR_FRAME_NODES: src = &c->d_nodes; n = (size_t)f.n_nodes * (f.width == 2 ? HJR_NODE2_F4 : HJR_NODE4_F4) * 16; break;
    case HJR_FRAME_TRI_GEOM: src = &c->d_tri_geom; n = (size_t)std::max(f.n_tris, 1u) * HJR_TRI_F4 * 16; break;
    case HJR_FRAME_TRI_SHADE: src = &c->d_tri_shade; n = (size_t)f.n_tris * HJR_SHADE_F4 * 16; break;
    case HJR_FRAME_LIGHTS: src = &c->d_lights; n = (size_t)f.n_lights * HJR_LIGHT_F4 * 16; break;
    default: set_error("hjr_copy_frame_data: unknown HJR_FRAME_* value"); return HJR_ERR_ARG;
    }
    *bytes = n;
    if (!dst || n == 0) return HJR_OK;
    if (dst_bytes < n) { set_error("hjr_copy_frame_data: destination too small"); return HJR_ERR_ARG; }
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipMemcpy(dst, src->p, n, hipMemcpyDeviceToHost));
    return HJR_OK;
}

extern "C" int hjr_set_transforms(hjr_ctx* c, const float* m, const float* inv, uint32_t n)
{
    const int rc = hjr_prepare_transforms(c, m, inv, n);
    return rc != HJR_OK ? rc : hjr_commit_transforms(c);
}

// hjr_set_lut / hjr_set_sky: an image of `texel` bytes per pixel into `buf`, its size into (cw, ch); a null or empty image switches it off
static int set_image(hjr_ctx* c, const char* who, DevBuf& buf, const void* rgba, int w, int h, size_t texel, int& cw, int& ch)
{
    HIPCHK(hipSetDevice(c->device));
    c->frame_gen++;
    c->tmp.have_prev = false; // temporal history: the shading / the lighting changes
    if (!rgba || w <= 0 || h <= 0) { cw = ch = 0; return HJR_OK; }
    if (!buf.upload(rgba, (size_t)w * (size_t)h * texel, c->stream)) { set_error(std::string(who) + ": upload failed"); return HJR_ERR_DEVICE; }
    HIPCHK(hipStreamSynchronize(c->stream));
    cw = w; ch = h;
    return HJR_OK;
}
extern "C" int hjr_set_lut(hjr_ctx* c, const uint8_t* rgba, int w, int h)
{
    if (!c) { set_error("hjr_set_lut: null context"); return HJR_ERR_ARG; }
    return set_image(c, "hjr_set_lut", c->d_lut, rgba, w, h, 4, c->lut_w, c->lut_h);
}
extern "C" int hjr_set_sky(hjr_ctx* c, const float* rgba, int w, int h)
{
    if (!c) { set_error("hjr_set_sky: null context"); return HJR_ERR_ARG; }
    return set_image(c, "hjr_set_sky", c->d_sky, rgba, w, h, 16, c->sky_w, c->sky_h);
}

static int fetch_stats(hjr_ctx* c, hipStream_t st)
{
    unsigned long long h[HJR_NSTAT];
    HIPCHK(hipMemcpyAsync(h, (char*)c->d_work.p + WorkArea::STATS, sizeof(h), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    uint64_t* dst = &c->stats.samples;
    for (int i = 0; i < 10; i++) dst[i] = h[i];
    c->stats.stack_overflow_pushes = h[10];
    { // option "firefly_clamp": the work area is zeroed before every launch, so a launch on which the rule did not act reads 0
        unsigned long long n = 0;
        HIPCHK(hipMemcpy(&n, (char*)c->d_work.p + WorkArea::FIREFLY, sizeof(n), hipMemcpyDeviceToHost));
        c->stats.firefly_clamped = n;
    }
    {
        unsigned long long nl[1 + HJR_NAN_LIST];
        HIPCHK(hipMemcpy(nl, (char*)c->d_work.p + WorkArea::NAN_LIST, sizeof(nl), hipMemcpyDeviceToHost));
        const uint32_t n = (uint32_t)std::min<unsigned long long>(nl[0], HJR_NAN_LIST);
        c->stats.nan_located = n;
        for (uint32_t i = 0; i < HJR_NAN_LIST; i++) {
            const unsigned long long k = i < n ? nl[1 + i] : 0ull;
            c->stats.nan_where[i][0] = (uint32_t)(k & 0x1fffu); c->stats.nan_where[i][1] = (uint32_t)((k >> 13) & 0x1fffu); c->stats.nan_where[i][2] = (uint32_t)(k >> 26);
        }
    }
#ifdef HJR_WF_TIMING
    { // diagnostic build only: where the waves of the wavefront kernel spend their clocks
        unsigned long long d[24];
        (void)hipMemcpyFromSymbol(d, HIP_SYMBOL(wf_diag), sizeof(d));
        const double tot = (double)d[0] + (double)d[1] + (double)d[2];
        if (tot > 0) {
            fprintf(stderr, "[hjr wf timing] scheduler idle %.1f%%  trace stage %.1f%% (hand-overs %.1f%%)  shade stage %.1f%% (waiting for context loads %.1f%%, store + push %.1f%%)\n",
                    100 * d[0] / tot, 100 * d[1] / tot, 100 * d[9] / tot, 100 * d[2] / tot, 100 * d[3] / tot, 100 * d[10] / tot);
            fprintf(stderr, "[hjr wf timing] shade batches %llu, %.1f contexts each; trace calls %llu, hand-overs %llu with %.1f finished rays each\n", d[4], d[4] ? (double)d[5] / d[4] : 0.0,
                    d[8], d[6], d[6] ? (double)d[7] / d[6] : 0.0);
            fprintf(stderr, "[hjr wf timing] trace stage lanes: outer iterations %llu with %.1f lanes holding a ray; node steps %llu wave-iterations x %.1f lanes; triangle tests %llu x %.1f lanes\n",
                    d[15], d[15] ? (double)d[16] / d[15] : 0.0, d[11], d[11] ? (double)d[12] / d[11] : 0.0, d[13], d[13] ? (double)d[14] / d[13] : 0.0);
            unsigned long long z[24] = { 0 };
            (void)hipMemcpyToSymbol(HIP_SYMBOL(wf_diag), z, sizeof(z));
        }
    }
#endif
#ifdef HJR_WF_WATCHDOG
    { // diagnostic build only: did the wavefront kernel run into its deadline, and where?
        unsigned long long wd[19];
        HIPCHK(hipMemcpy(wd, (char*)c->d_work.p + WorkArea::DIAG, sizeof(wd), hipMemcpyDeviceToHost));
        unsigned int where[8] = { 0 };
        (void)hipMemcpyFromSymbol(where, HIP_SYMBOL(wf_where), sizeof(where));
        if (where[1] | where[2] | where[3] | where[4] | where[5] | where[6]) {
            fprintf(stderr, "[hjr wf watchdog] deadline hit in (lane counts): take %u, push slot-wait %u, push publish-wait %u, trace loop %u, pop %u, scheduler %u\n", where[1], where[2], where[3], where[4], where[5], where[6]);
            fprintf(stderr, "[hjr wf watchdog] first workgroup to give up: block %llu live %llu items_held %llu\n", wd[17], wd[16], wd[18]);
            for (int q = 0; q < 5; q++) fprintf(stderr, "   queue %d: commit %llu head %llu tail %llu\n", q, wd[1 + q], wd[6 + q], wd[11 + q]);
            unsigned int zero[8] = { 0 };
            (void)hipMemcpyToSymbol(HIP_SYMBOL(wf_where), zero, sizeof(zero));
        }
    }
#endif
#ifdef HJR_TIMING
    { // diagnostic build only: wave-clock shares of the megakernel's loop phases and lane occupancies
        unsigned long long tk[25];
        HIPCHK(hipMemcpy(tk, (char*)c->d_work.p + WorkArea::DIAG, sizeof(tk), hipMemcpyDeviceToHost));
        const double tot = (double)tk[0] + (double)tk[1] + (double)tk[2];
        if (tot > 0) fprintf(stderr, "[hjr timing] roulette/refill/regeneration %.1f%%  fused trace %.1f%%  resolve + hit program + shading %.1f%%  (%.3g wave-clocks)\n",
                             100 * tk[0] / tot, 100 * tk[1] / tot, 100 * tk[2] / tot, tot);
        if (tk[3]) fprintf(stderr, "[hjr timing] lanes per round: closest-hit ray %.1f, shadow ray %.1f, serviced %.1f\n", (double)tk[4] / tk[3], (double)tk[5] / tk[3], (double)tk[6] / tk[3]);
        const unsigned long long* td = tk + 7;
        if (td[0]) fprintf(stderr, "[hjr timing] traversal: %.1f passes per round, %.1f lanes with a ray per pass (%.1f on a shadow ray); node steps %.2f wave-iterations per pass x %.1f lanes; "
                                   "leaf parts in %.0f%% of the passes x %.1f lanes; triangle tests %.2f wave-iterations per pass x %.1f lanes\n",
                           tk[3] ? (double)td[0] / tk[3] : 0.0, (double)td[1] / td[0], (double)td[8] / td[0], (double)td[2] / td[0], td[2] ? (double)td[3] / td[2] : 0.0,
                           100.0 * td[4] / td[0], td[4] ? (double)td[5] / td[4] : 0.0, (double)td[6] / td[0], td[6] ? (double)td[7] / td[6] : 0.0);
        const unsigned long long* ls = tk + 17; // (rounds that reach the site, rounds of those with at most 32 drawing lanes) x (light sample, Disney / glass sample, first walk step, roulette)
        if (tk[3]) fprintf(stderr, "[hjr timing] draw sites: rounds %llu light %llu %llu bsdf %llu %llu walk %llu %llu roulette %llu %llu\n", tk[3], ls[0], ls[1], ls[2], ls[3], ls[4], ls[5], ls[6], ls[7]);
    }
#endif
    return HJR_OK;
}

extern "C" int hjr_synchronize(hjr_ctx* c)
{
    if (!c) { set_error("hjr_synchronize: null context"); return HJR_ERR_ARG; }
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipDeviceSynchronize());
    return HJR_OK;
}

extern "C" int hjr_get_stats(hjr_ctx* c, hjr_stats* out)
{
    if (!c || !out) { set_error("hjr_get_stats: null argument"); return HJR_ERR_ARG; }
    uint32_t out_size;
    if (!hjr::abi_size(out, out_size, "hjr_get_stats")) return HJR_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    if (c->event_pending) {
        HIPCHK(hipEventSynchronize(c->ev1));
        float ms = 0.0f;
        HIPCHK(hipEventElapsedTime(&ms, c->ev0, c->ev1));
        c->stats.last_kernel_ms = ms;
        c->event_pending = false;
        if (c->d_work.p) { int rc = fetch_stats(c, c->stream); if (rc != HJR_OK) return rc; }
    }
    return hjr::abi_give(out, c->stats, "hjr_get_stats") ? HJR_OK : HJR_ERR_ARG; // sized struct: at most out->struct_size bytes are written
}

#ifdef HJR_UNITY /* the other units of the device layer and the render kernels' units: hjr_render.hip declares what those instantiate, and hjr_launch_trace.hip compiles the hook's kernels with the hook's header, so it goes ahead of hjr_util.hip */
#include "hjr_render.hip"
#include "hjr_post.hip"
#ifdef HJR_LEAN_VARIANT /* NEE without the statistics counters only; every other launch runs that kernel too (timing experiments, not pictures) */
template int hjr_launch<HJR_INTEGRATOR_NEE, false>(hjr_ctx*, const LaunchPlan&, uint64_t, hipStream_t);
#else
#include "hjr_launch_nee.hip"
#include "hjr_launch_pt.hip"
#include "hjr_launch_mis.hip"
#include "hjr_launch_trace.hip"
#endif
#include "hjr_util.hip"
#endif
