// Stand-alone test (own main, built with -fsanitize=address,undefined by tests/test_deform_host.py) of the host half of hjr_set_morph
// (henjou-renderer_amd/host/frame.cpp): the validation of the sets, the blend on the worker threads and the per-vertex blend the device
// builder's light table uses.  Shapes of the GPU tests: a set whose first vertex and size are no multiples of 64, a set that ends at the
// scene's last vertex, K = 1 and K = 5, two sets sharing one weight, weights holding 0, a negative value and one above 1; and a set large
// enough for several worker chunks.  The blend is compared with a scalar restatement of the rule, so the program must be compiled with
// -ffp-contract=off like the unit it tests.
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../../henjou-renderer_amd/host/frame.hpp"

using namespace hjr;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); fails++; } } while (0)

struct Case {
    uint32_t first, n, K, fw;
    bool normals;
    std::vector<float> pd, nd;
};

int main()
{
    const uint32_t NV = 200000; // several chunks of 3 * 16384 components in the large set
    std::mt19937 rng(17);
    std::uniform_real_distribution<float> U(-1.0f, 1.0f);
    SceneCopy sc;
    sc.vertices.resize(3 * (size_t)NV); sc.normals.resize(3 * (size_t)NV);
    for (float& x : sc.vertices) x = 3.0f * U(rng);
    for (float& x : sc.normals) x = U(rng);
    std::vector<Case> cases = { { 37, 601, 5, 1, true, {}, {} }, { 1000, 6, 1, 0, false, {}, {} }, { 2000, 150001, 3, 6, true, {}, {} }, { NV - 203, 203, 1, 0, false, {}, {} } };
    const std::vector<float> w = { 1.25f, 0.0f, -0.5f, 0.75f, 1.5f, 0.3f, 0.9f, -0.1f, 2.0f };
    std::vector<hjr_morph_set> sets;
    for (Case& c : cases) {
        c.pd.resize(3 * (size_t)c.K * c.n);
        for (float& x : c.pd) x = 0.3f * U(rng);
        if (c.normals) { c.nd.resize(c.pd.size()); for (float& x : c.nd) x = 0.3f * U(rng); }
        sets.push_back({ c.first, c.n, c.K, c.fw, c.pd.data(), c.normals ? c.nd.data() : nullptr });
    }
    hjr_morph m;
    HJR_INIT(m);
    m.n_sets = (uint32_t)sets.size(); m.n_weights = (uint32_t)w.size(); m.sets = sets.data(); m.default_weights = w.data();
    Morph mo;
    std::string err;
    CHECK(mo.set(m, NV, err));
    CHECK(mo.active() && mo.sets.size() == sets.size() && mo.weights == w && mo.n_vertices == 601u + 6u + 150001u + 203u);

    // the rule, scalar: p = p + w[k] * d[k] in target order, the product rounded, then the sum
    std::vector<float> ev = sc.vertices, en = sc.normals;
    for (const Case& c : cases)
        for (uint32_t i = 0; i < c.n; i++)
            for (int a = 0; a < 3; a++) {
                const size_t at = 3 * ((size_t)c.first + i) + a;
                for (uint32_t k = 0; k < c.K; k++) {
                    volatile float t = w[c.fw + k] * c.pd[3 * ((size_t)k * c.n + i) + a];
                    ev[at] = ev[at] + t;
                    if (c.normals) { volatile float u = w[c.fw + k] * c.nd[3 * ((size_t)k * c.n + i) + a]; en[at] = en[at] + u; }
                }
            }
    std::vector<float> v1, n1, v16, n16;
    set_host_threads(1);
    morph_blend(sc, mo, mo.weights.data(), v1, n1);
    set_host_threads(16);
    morph_blend(sc, mo, mo.weights.data(), v16, n16);
    set_host_threads(0);
    CHECK(v1.size() == ev.size() && memcmp(v1.data(), ev.data(), ev.size() * 4) == 0);
    CHECK(n1.size() == en.size() && memcmp(n1.data(), en.data(), en.size() * 4) == 0);
    CHECK(memcmp(v1.data(), v16.data(), v1.size() * 4) == 0 && memcmp(n1.data(), n16.data(), n1.size() * 4) == 0); // 1 and 16 threads: identical bytes
    // one vertex at a time (the device builder's light table): inside every set, at its ends, and outside
    for (uint32_t vtx : { 0u, 36u, 37u, 637u, 638u, 1000u, 1005u, 1006u, 2000u, 152000u, 152001u, NV - 204, NV - 203, NV - 1 }) {
        float p[3], n[3];
        morph_vertex(sc, mo, mo.weights.data(), vtx, p, n);
        CHECK(memcmp(p, &ev[3 * (size_t)vtx], 12) == 0 && memcmp(n, &en[3 * (size_t)vtx], 12) == 0);
    }

    // validation: an error names its cause and leaves the morph as it was
    auto refused = [&](hjr_morph bad, const char* words) {
        Morph keep = mo;
        std::string e;
        const bool ok = mo.set(bad, NV, e);
        CHECK(!ok && e.find(words) != std::string::npos);
        if (ok || e.find(words) == std::string::npos) printf("  got: %s\n", e.c_str());
        CHECK(mo.sets.size() == keep.sets.size() && mo.deltas == keep.deltas && mo.weights == keep.weights);
    };
    std::vector<hjr_morph_set> b = sets;
    hjr_morph bad = m;
    bad.sets = b.data();
    b[3].first_vertex = NV - 202; refused(bad, "outside the scene"); b = sets;                // one vertex past the end
    b[1].first_vertex = 637; refused(bad, "overlapping"); b = sets;                            // the last vertex of set 0
    b[2].first_vertex = 1005; refused(bad, "overlapping"); b = sets;
    b[0].first_weight = 5; refused(bad, "n_weights"); b = sets;                                // 5 + 5 > 9
    b[0].position_deltas = nullptr; refused(bad, "null position_deltas"); b = sets;
    b[0].n_vertices = 0; refused(bad, "no vertices"); b = sets;
    bad.sets = nullptr; refused(bad, "null sets"); bad.sets = b.data();
    b[1].first_vertex = 638; // adjacent to set 0: accepted
    CHECK(mo.set(bad, NV, err));
    b = sets;
    bad.default_weights = nullptr; // zeros
    CHECK(mo.set(bad, NV, err) && mo.weights == std::vector<float>(w.size(), 0.0f));
    bad.n_sets = 0; // removes the morph
    CHECK(mo.set(bad, NV, err) && !mo.active() && mo.deltas.empty());
    if (fails) { printf("morph_blend_test: %d check(s) failed\n", fails); return 1; }
    printf("morph_blend_test ok\n");
    return 0;
}
