// Per-frame host set-up that replaces the reference's GAS/IAS build (renderer/renderer.h:319-490) and hoists the
// per-hit vertex/normal transforms of __closesthit__ch and light_sample (light_sample.h:43-58) to once per frame:
// instances are flattened to world space, a binned-SAH BVH2 is built over all triangles, and the light table is
// pre-transformed.  The arithmetic of every value the kernel consumes is the reference's (fp32, same order).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/henjou_hip.h"
#include "../csrc/hjr_layout.h"
#include "options.hpp"

namespace hjr {

struct FrameData {
    std::vector<float> nodes;      // HJR_NODE2_F4 / HJR_NODE4_F4 float4 per inner node
    std::vector<float> tri_geom;   // HJR_TRI_F4 float4 per triangle, leaf order
    std::vector<float> tri_shade;  // HJR_SHADE_F4 float4 per triangle, global prim order
    std::vector<uint32_t> tri_inst;// instance id per global prim
    std::vector<float> lights;     // HJR_LIGHT_F4 float4 per emissive triangle
    uint32_t n_tris = 0, n_nodes = 0, n_lights = 0, depth = 0;
    uint32_t stack_need = 2; // worst-case traversal stack entries per lane for this tree
    uint32_t width = 2;      // 2 or 4 (node format, hjr_layout.h)
    int lds_mode = 0;        // 0: nodes/triangles read from memory; 1: staged in LDS, 32-bit stack entries; 2: 16-bit entries
};

// Owning copy of an hjr_scene_view (cpySceneDataToDevice keeps the host vectors alive too, renderer.h:197-255).
struct SceneCopy {
    std::vector<float> vertices, normals, texcoords, light_prim_emission;
    std::vector<uint32_t> indices, material_ids, prim_offset, light_prim_ids;
    std::vector<hjr_material> materials;
    struct Tex { uint32_t offset, width, height; int srgb; }; // offset in texels into `texels`
    std::vector<Tex> textures;
    std::vector<uint32_t> texels; // RGBA8 atlas, all textures back to back
    uint32_t n_triangles = 0, n_instances = 0;
    bool set(const hjr_scene_view& v, std::string& err);
};

// Owning copy of an hjr_morph (include/henjou_hip.h, "deforming meshes"): the sets in the caller's order, every set's deltas
// in one array (the device builder uploads it as it is), the weights as last set.
struct MorphSet {
    uint32_t first_vertex, n_vertices, n_targets, first_weight;
    size_t pos, nrm; // first float of the set's position / normal deltas in Morph::deltas (target-major); nrm == Morph::NONE: normals stay at the base
};
struct Morph {
    static constexpr size_t NONE = ~(size_t)0;
    std::vector<MorphSet> sets;
    std::vector<float> deltas, weights;
    uint32_t n_vertices = 0; // vertices of all sets
    bool active() const { return !sets.empty(); }
    // validates against a scene of `scene_vertices` vertices and copies; an error (range outside the scene, overlapping sets, weights outside
    // n_weights, null pointers) leaves *this as it was.  m.n_sets == 0 removes the morph
    bool set(const hjr_morph& m, uint32_t scene_vertices, std::string& err);
};
// the blend rule of include/henjou_hip.h for one component: p = p + w[k] * d[k] in target order (this unit is compiled with -ffp-contract=off)
inline float morph_component(float base, const float* d, size_t stride, const float* w, uint32_t K)
{
    float p = base;
    for (uint32_t k = 0; k < K; k++) { const float t = w[k] * d[(size_t)k * stride]; p = p + t; }
    return p;
}
// the whole scene under the weights `w` (Morph::weights' size) into vert / norm: base bytes outside the sets.  Worker threads; the output does
// not depend on their number (element-wise)
void morph_blend(const SceneCopy& sc, const Morph& mo, const float* w, std::vector<float>& vert, std::vector<float>& norm);
// one vertex of it: p[3], n[3]
void morph_vertex(const SceneCopy& sc, const Morph& mo, const float* w, uint32_t vertex, float* p, float* n);

// bo.allow_lds: let small scenes use the LDS-resident BVH2 layout; the other fields force a layout / leaf size (tests, tuning)
// vert / norm: the working copy of a morphed scene (morph_blend) in place of sc.vertices / sc.normals; null: those
bool build_frame(const SceneCopy& sc, const float* transforms12, const float* inv12, uint32_t n_instances, const BuildOptions& bo,
                 FrameData& out, std::string& err, const float* vert = nullptr, const float* norm = nullptr);

// the light table of build_frame alone (out.lights, out.n_lights).  vert / norm as above; else with `mo` and `w` only the light triangles'
// vertices are blended (morph_vertex), which is what the device builder's prepare needs: O(lights x targets)
void build_lights(const SceneCopy& sc, const float* transforms12, const float* inv12, FrameData& out, const float* vert = nullptr,
                  const float* norm = nullptr, const Morph* mo = nullptr, const float* w = nullptr);

} // namespace hjr
