// Device buffers of a context and the per-frame device BVH4 builder (option "device_bvh", csrc/hjr_bvh_build.hip).
// Kept free of the kernel headers so that hjr_bvh_build.hip compiles on its own.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

// Owns its allocation.  The one condition: a DevBuf is destroyed (or released, or moved onto) with its device current, which every entry
// point and hjr_destroy see to before they touch a context.
struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept { swap(o); }
    DevBuf& operator=(DevBuf&& o) noexcept { release(); swap(o); return *this; }
    ~DevBuf() { release(); }
    template <class T> T* as() const { return static_cast<T*>(p); }
    // grow without copying to exactly `bytes` (the old contents are lost); *grown tells whether the buffer was reallocated
    bool reserve(size_t bytes, bool* grown = nullptr)
    {
        if (grown) *grown = cap < bytes;
        if (cap >= bytes) return true;
        release();
        if (hipMalloc(&p, bytes) != hipSuccess) return false;
        cap = bytes;
        return true;
    }
    bool upload(const void* src, size_t bytes, hipStream_t st) // grows with 25 % slack
    {
        if (bytes > cap && !reserve(bytes + bytes / 4 + 256)) return false;
        return !bytes || hipMemcpyAsync(p, src, bytes, hipMemcpyHostToDevice, st) == hipSuccess;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
    void swap(DevBuf& o) { std::swap(p, o.p); std::swap(cap, o.cap); }
};

namespace hjr {
struct SceneCopy;

// Traversal-stack entries a device-built tree may need: the tile classifier takes 64 * stack_need * 4 bytes of dynamic LDS without
// raising the kernel's limit (hjr_render.hip::order_tiles), which stays at 32 KB with this cap.
constexpr uint32_t DEVICE_BVH_MAX_STACK = 128;
// Option "device_bvh_instances": instance subtrees one top tree takes (its clusters live in the LDS of one workgroup)
constexpr uint32_t HJR_TOP_MAX = 1024;

struct DeviceBvh {
    // object-space scene, uploaded at the first device build after hjr_upload_scene (have_scene = false drops it)
    DevBuf vert, norm, uv, idx, mat, prim_off;
    bool have_scene = false;
    DevBuf xf;  // per instance: 12 floats of the transform, then 12 of the inverse
    // scratch of one build
    DevBuf wv, box, cent, keys[2], vals[2], hist, part, leaf_box, inner_box, inner_child, inner_range, parent, counter, frontier[2], wide, hdr;
    DevBuf node_count, node_cost, leaf_pos; // scratch of the treelet restructuring ("device_bvh_opt")
    // the frame data a build writes; hjr_commit_transforms swaps them with the context's current buffers when the build succeeds
    DevBuf nodes, tri_geom, tri_shade, tri_inst, lights;
    DevBuf stage; // option "device_bvh_graft": a commit's skeleton nodes at their skeleton ids, before the top-node count is known
    // Option "device_bvh_instances": the BVH2 whose subtrees are the instances, built once per uploaded scene and build tag and kept
    // between commits.  A commit rewrites only the k - 1 `top` nodes above the instance roots (child, range, parent of their children).
    struct Topology {
        DevBuf child, range, parent;  // per inner node (first row, triangles) | parent: inner nodes, then the sorted leaves
        DevBuf pos, order;            // per sorted leaf: its tri_geom row, its triangle
        DevBuf top, top_ids;          // per inner node: 1 above the instance roots | those nodes' ids, ascending (the root first)
        DevBuf root, list;            // per instance: BVH2 ref of its subtree | the non-empty instances, ascending
        DevBuf bounds;                // scratch of the build: per instance centroid bounds
        // Option "device_bvh_graft": the BVH4 collapse of every instance subtree of more than leaf_max triangles ("skeleton"), made once
        // from the object-space boxes; ids breadth-first over all instances together.  With it only pos, order, list and these are kept.
        DevBuf skel_refs, skel_parent; // per skeleton node: refs row (inner refs are skeleton ids) | 4 * parent + slot (0xffffffff: an instance root)
        DevBuf inst_ref, inst_stat;    // per non-empty instance: skeleton id of its root, or its leaf ref (<= leaf_max triangles) | worst pending entries, largest leaf depth below its root
        DevBuf top_box;                // scratch of a commit: boxes of the k instances, then of the k - 1 binary top nodes
        bool graft = false, skel_deep = false; // built with the skeleton | a skeleton deeper than the traversal stack: commits take the ordinary build
        uint32_t n_skel = 0;           // skeleton nodes
        bool valid = false;
        uint32_t tag = 0, k = 0;      // build tag it was built under, non-empty instances
        float ms = 0.0f;              // HIP-event time of its build
    } topo;
    void drop_topology() { topo = Topology(); }
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    void release(); // what is not a DevBuf: the events (the buffers go with the struct)
};

// hjr_set_morph on the device builder: the deltas and the set table go up once, the weights per commit, and
// hjr_morph_kernel writes the working vertex / normal arrays that every flatten of the three paths below reads in place of b.vert / b.norm.
// Nothing here is allocated without a morph.  The context keeps it beside the DeviceBvh and hands it to every build.
struct Morph;
struct DeviceMorph {
    const Morph* host = nullptr;   // the context's morph (null or not active: the builds read the base arrays)
    const float* w_next = nullptr; // the weights of this commit, host->weights' size
    DevBuf vert, norm;             // working arrays, the base's size
    DevBuf deltas, table, weights; // Morph::deltas | one record per set | the weights of the working arrays
    bool uploaded = false;         // deltas and table are the host's
    bool copied = false;           // the working arrays hold the base outside the sets (and what the last blend wrote inside them)
    bool blended = false;          // ... and inside the sets the blend of the base under `w`
    std::vector<float> w;
    uint32_t launched = 0;         // vertices hjr_morph_kernel was launched over since the caller zeroed it
    hipEvent_t ev0 = nullptr, ev1 = nullptr; // around that launch on the build's stream (kernel_ms reads them after the build's host wait)
    float kernel_ms() const { float ms = 0.0f; return launched && ev0 && hipEventElapsedTime(&ms, ev0, ev1) == hipSuccess ? ms : 0.0f; }
    void drop() // with the device current, like every DevBuf
    {
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
        *this = DeviceMorph();
    }
};

struct DeviceBvhResult {
    uint32_t n_nodes = 0, stack_need = 0, depth = 0;
    float build_ms = 0.0f; // HIP-event time of the build's kernels
    float sah = 0.0f;      // BVH4 SAH of the nodes, computed on the device in a fixed summation order (0: empty scene)
    uint32_t instances = 0; // device_bvh_instances: instance subtrees under the top tree (0: an ordinary build)
    bool too_deep = false;  // the error is "BVH deeper than the traversal stack"
};

// Enqueues the whole build on `st` behind whatever is already there, waits for it and reads back its header.  HJR_ERR_ARG with `err`
// set for a scene the host builder rejects too (non-finite vertex, tree deeper than the traversal stack allows), HJR_ERR_DEVICE for a
// runtime failure.  The lights are the host's table (build_lights), copied into `b.lights`.
// `dm` (all three builds; may be null): the morph of the scene, blended ahead of the flatten when its working arrays are not current.
// `opt_rounds` (option "device_bvh_opt", 0..3) treelet-restructuring rounds run over the BVH2 before the collapse; 0 leaves the build as it was.
int device_bvh_build(DeviceBvh& b, const SceneCopy& sc, const float* M, const float* Mi, uint32_t n_inst, uint32_t leaf_max, uint32_t opt_rounds,
                     const float* lights, size_t light_floats, hipStream_t st, DeviceBvhResult& r, std::string& err, DeviceMorph* dm = nullptr);
// Option "device_bvh_refit": the frame data for new transforms over the topology of the CURRENT frame data (`cur_nodes`, `cur_geom`: a
// device build or refit of the same scene with n_nodes nodes; only the refs rows and the prim ids are read, nothing is written there).
// Flatten in leaf order, node boxes bottom-up over the BVH4, tree cost; one host wait.  Writes b.nodes / tri_* / lights like the build;
// r.stack_need and r.depth stay 0 (the topology's, which the caller has).  Errors as device_bvh_build; HJR_ERR_DEVICE when the current
// data fails a bound.  At least 2 triangles.
int device_bvh_refit(DeviceBvh& b, const SceneCopy& sc, const float* M, const float* Mi, uint32_t n_inst, const DevBuf& cur_nodes, const DevBuf& cur_geom,
                     uint32_t n_nodes, const float* lights, size_t light_floats, hipStream_t st, DeviceBvhResult& r, std::string& err, DeviceMorph* dm = nullptr);
// Option "device_bvh_instances": the frame data for these transforms from per-instance trees.  The topology (a BVH2 over object-space
// boxes whose subtrees are the instances: sort keys carry the instance id above the Morton code; `opt_rounds` treelet rounds that never
// cross an instance) is built when b.topo is not valid for `tag`, and kept.  Every call flattens in its leaf order, computes the world
// boxes inside the instance subtrees, builds the top tree over the instance boxes in one workgroup, collapses and costs like a build.
// No non-empty instance, more than HJR_TOP_MAX of them, or a tree deeper than the traversal stack: device_bvh_build runs instead
// (r.instances == 0).  Writes and errors as device_bvh_build.
// `graft` (option "device_bvh_graft"): the topology also holds every instance's BVH4, collapsed once by object-space areas; a commit
// flattens, refits those nodes bottom-up (device_bvh_refit's climb), builds and collapses the top tree over the instance boxes in one
// workgroup and places the instance nodes behind the top nodes.  No per-level launches, one host wait; the BVH2 is freed after the
// topology build.  The same fallbacks.
int device_bvh_instances(DeviceBvh& b, const SceneCopy& sc, const float* M, const float* Mi, uint32_t n_inst, uint32_t leaf_max, uint32_t opt_rounds,
                         uint32_t tag, bool graft, const float* lights, size_t light_floats, hipStream_t st, DeviceBvhResult& r, std::string& err,
                         DeviceMorph* dm = nullptr);
} // namespace hjr
