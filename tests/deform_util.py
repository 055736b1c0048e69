"""Helpers of the deformation tests (hjr_update_vertices, hjr_set_morph): the blend rule restated in numpy, seeded
morph sets over the bundled scene, a generated glTF with one morphed mesh and a `weights` channel, and an independent reading of it.

The rule (include/henjou_hip.h): per vertex and component, in fp32, p = base; p = p + w[k] * d[k] for k = 0 .. K-1, the product rounded,
then the sum.  numpy's float32 arithmetic rounds every operation, so the loop below is that rule to the bit."""
import base64
import json
import os

import numpy as np

F32 = np.float32


def blend(base, deltas, w):
    """base [n, 3], deltas [K, n, 3], w [K]: the rule above."""
    p = np.array(base, dtype=F32)
    for k in range(len(deltas)):
        p = p + F32(w[k]) * np.asarray(deltas[k], dtype=F32)
    return p


def apply_morph(arrays, sets, weights):
    """A copy of the scene arrays with every set blended under `weights` (float32 [n_weights]); vertices outside the sets keep the base
    bytes, and so do the normals of a set without normal deltas."""
    a = dict(arrays)
    v = np.array(arrays["vertices"], dtype=F32).reshape(-1, 3)
    n = np.array(arrays["normals"], dtype=F32).reshape(-1, 3)
    weights = np.asarray(weights, dtype=F32)
    for s in sets:
        pd = np.asarray(s["position_deltas"], dtype=F32)
        f, cnt, K, fw = int(s["first_vertex"]), pd.shape[1], pd.shape[0], int(s.get("first_weight", 0))
        v[f:f + cnt] = blend(v[f:f + cnt], pd, weights[fw:fw + K])
        if s.get("normal_deltas") is not None:
            n[f:f + cnt] = blend(n[f:f + cnt], s["normal_deltas"], weights[fw:fw + K])
    a["vertices"], a["normals"] = v.reshape(-1), n.reshape(-1)
    return a


def n_morph_vertices(sets):
    return sum(np.asarray(s["position_deltas"]).shape[1] for s in sets)


def instance_vertex_range(arrays, inst):
    """[first, end) of the vertices instance `inst` indexes; the loader de-indexes, so an instance owns a contiguous range."""
    po = np.asarray(arrays["prim_offsets"], dtype=np.int64)
    n_tris = np.asarray(arrays["indices"]).size // 3
    t0, t1 = int(po[inst]), int(po[inst + 1]) if inst + 1 < po.size else n_tris
    idx = np.asarray(arrays["indices"], dtype=np.int64)[3 * t0:3 * t1]
    return int(idx.min()), int(idx.max()) + 1


def light_instance(arrays):
    po = np.asarray(arrays["prim_offsets"], dtype=np.int64)
    return int(np.searchsorted(po, int(arrays["light_prim_ids"][0]), side="right") - 1)


def scene_extent(arrays):
    v = np.asarray(arrays["vertices"], dtype=F32).reshape(-1, 3)
    return float((v.max(0) - v.min(0)).max())


def make_set(rng, first_vertex, n_vertices, K, first_weight, scale, normals):
    s = {"first_vertex": int(first_vertex), "first_weight": int(first_weight),
         "position_deltas": (rng.uniform(-1.0, 1.0, (K, n_vertices, 3)) * scale).astype(F32)}
    if normals:
        s["normal_deltas"] = rng.uniform(-0.3, 0.3, (K, n_vertices, 3)).astype(F32)
    return s


def standard_sets(arrays, seed=7):
    """The sets of the bundled scene the GPU tests share, and their weights.  Deltas about a tenth of the box.
      A  the instance that holds the emissive triangles, K = 1, weight 0 (shared with C);
      B  first_vertex 37 and 601 vertices (neither a multiple of 64; three workgroups of 256), K = 5 with normal deltas, weights 1..5:
         a remainder behind any unroll by 2 or 4;
      C  the last 203 vertices of the scene, K = 1, weight 0.
    The weights hold 0, a negative value and one above 1."""
    rng = np.random.default_rng(seed)
    nv = np.asarray(arrays["vertices"]).size // 3
    scale = 0.1 * scene_extent(arrays)
    l0, l1 = instance_vertex_range(arrays, light_instance(arrays))
    b0, bn, cn = 37, 601, 203
    assert (l1 <= b0 or l0 >= b0 + bn) and b0 + bn <= nv - cn and (l1 <= nv - cn), "the bundled scene changed: the sets would overlap"
    assert b0 % 64 and bn % 64
    sets = [make_set(rng, l0, l1 - l0, 1, 0, scale, False), make_set(rng, b0, bn, 5, 1, scale, True), make_set(rng, nv - cn, cn, 1, 0, scale, False)]
    weights = np.array([1.25, 0.0, -0.5, 0.75, 1.5, 0.3], dtype=F32)
    return sets, weights


WEIGHT_SEQUENCE = np.array([[1.25, 0.0, -0.5, 0.75, 1.5, 0.3],
                            [1.0, 0.2, -0.4, 0.7, 1.4, 0.35],
                            [0.8, 0.4, -0.3, 0.65, 1.3, 0.4],
                            [0.6, 0.6, -0.2, 0.6, 1.2, 0.45]], dtype=F32)  # four frames of a deformation that moves a little per frame


def changed_fraction(a, b):
    """share of the pixels in which two colour images differ"""
    a, b = np.asarray(a, dtype=F32), np.asarray(b, dtype=F32)
    return float(np.mean(np.any(a.view(np.uint32) != b.view(np.uint32), axis=-1)))


def world_vertices_by_prim(dev, hjr):
    """[n_tris, 9] world vertices of hjr_copy_frame_data's tri_geom rows, in global prim order"""
    g = dev.copy_frame_data(hjr.FRAME_TRI_GEOM).reshape(-1, 12)
    prim = g[:, 9].view(np.uint32)
    return g[np.argsort(prim, kind="stable")][:, :9]


# ------------------------------------------------------------------------------------------------------------------ generated glTF

def write_morph_gltf(src_dir, dst_dir, name="cornell_morph.gltf", seed=11, K=2):
    """The bundled cornelbox.gltf with morph targets on the mesh of its node `node` (every primitive of that mesh gets K targets with
    POSITION, the first primitive also NORMAL), default `mesh.weights`, and one animation channel with "path": "weights".  The deltas are
    appended to a copy of the .bin.  Returns the description an independent reading needs:
    {"mesh": id, "node": id, "K": K, "defaults": [...], "times": [...], "values": [[K floats] per key]}."""
    rng = np.random.default_rng(seed)
    g = json.load(open(os.path.join(src_dir, "cornelbox.gltf")))
    buf = bytearray(open(os.path.join(src_dir, g["buffers"][0]["uri"]), "rb").read())
    pos_acc = lambda prim: g["accessors"][prim["attributes"]["POSITION"]]  # noqa: E731
    # the mesh with the most primitives that a node instantiates (they share the node's weights), the most vertices among equals
    nodes_with_mesh = [(i, n["mesh"]) for i, n in enumerate(g["nodes"]) if "mesh" in n]
    node, mesh = max(nodes_with_mesh, key=lambda nm: (len(g["meshes"][nm[1]]["primitives"]), sum(pos_acc(p)["count"] for p in g["meshes"][nm[1]]["primitives"])))
    extent = 0.0
    for p in g["meshes"][mesh]["primitives"]:
        a = pos_acc(p)
        extent = max(extent, max(hi - lo for lo, hi in zip(a["min"], a["max"])))

    def add_accessor(data, typ):
        while len(buf) % 4:
            buf.append(0)
        off = len(buf)
        buf.extend(np.ascontiguousarray(data, dtype="<f4").tobytes())
        g["bufferViews"].append({"buffer": 0, "byteOffset": off, "byteLength": data.size * 4})
        acc = {"bufferView": len(g["bufferViews"]) - 1, "componentType": 5126, "count": int(data.shape[0]), "type": typ}
        if typ == "VEC3":
            acc["min"], acc["max"] = [float(x) for x in data.min(0)], [float(x) for x in data.max(0)]
        g["accessors"].append(acc)
        return len(g["accessors"]) - 1

    for pi, p in enumerate(g["meshes"][mesh]["primitives"]):
        cnt = pos_acc(p)["count"]
        p["targets"] = []
        for _ in range(K):
            t = {"POSITION": add_accessor((rng.uniform(-1, 1, (cnt, 3)) * 0.15 * extent).astype(F32), "VEC3")}
            if pi == 0:
                t["NORMAL"] = add_accessor(rng.uniform(-0.3, 0.3, (cnt, 3)).astype(F32), "VEC3")
            p["targets"].append(t)
    defaults = [0.25, -0.5][:K] + [0.0] * max(0, K - 2)
    g["meshes"][mesh]["weights"] = defaults
    times = np.array([0.05, 0.1, 0.2], dtype=F32)
    values = np.array([[0.0, 1.0], [1.0, -0.5], [0.5, 1.5]], dtype=F32)[:, :K] if K <= 2 else rng.uniform(-0.5, 1.5, (3, K)).astype(F32)
    t_acc = add_accessor(times.reshape(-1, 1), "SCALAR")
    g["accessors"][t_acc]["min"], g["accessors"][t_acc]["max"] = [float(times.min())], [float(times.max())]
    v_acc = add_accessor(values.reshape(-1, 1), "SCALAR")
    anim = {"channels": [], "samplers": []}
    g.setdefault("animations", []).append(anim)
    anim["samplers"].append({"input": t_acc, "output": v_acc, "interpolation": "LINEAR"})
    anim["channels"].append({"sampler": 0, "target": {"node": node, "path": "weights"}})
    g["buffers"][0]["uri"] = name.replace(".gltf", ".bin")
    g["buffers"][0]["byteLength"] = len(buf)
    os.makedirs(dst_dir, exist_ok=True)
    open(os.path.join(dst_dir, g["buffers"][0]["uri"]), "wb").write(bytes(buf))
    json.dump(g, open(os.path.join(dst_dir, name), "w"))
    return {"mesh": mesh, "node": node, "K": K, "defaults": defaults, "times": [float(t) for t in times], "values": values.tolist()}


def _accessor(g, buf, i):
    a = g["accessors"][i]
    assert a["componentType"] == 5126 and "sparse" not in a
    bv = g["bufferViews"][a["bufferView"]]
    comps = {"SCALAR": 1, "VEC2": 2, "VEC3": 3, "VEC4": 4}[a["type"]]
    off = bv.get("byteOffset", 0) + a.get("byteOffset", 0)
    stride = bv.get("byteStride", 0) or comps * 4
    out = np.zeros((a["count"], comps), dtype=F32)
    for r in range(a["count"]):
        out[r] = np.frombuffer(buf, dtype="<f4", count=comps, offset=off + r * stride)
    return out


def _indices(g, buf, i):
    a = g["accessors"][i]
    bv = g["bufferViews"][a["bufferView"]]
    dt = {5121: "<u1", 5123: "<u2", 5125: "<u4"}[a["componentType"]]
    return np.frombuffer(buf, dtype=dt, count=a["count"], offset=bv.get("byteOffset", 0) + a.get("byteOffset", 0)).astype(np.int64)


def read_morph_gltf(path):
    """Independent reading of a glTF's morph data: per primitive of every mesh with targets, in file order, the de-indexed deltas
    ({"mesh", "primitive", "position_deltas" [K, n, 3], "normal_deltas" or None}), the default weights per mesh, and the weight keys of
    every `weights` channel ({"mesh", "times", "values" [keys, K]})."""
    g = json.load(open(path))
    uri = g["buffers"][0]["uri"]
    buf = base64.b64decode(uri.split(",", 1)[1]) if uri.startswith("data:") else open(os.path.join(os.path.dirname(path), uri), "rb").read()
    prims, defaults, tracks = [], {}, []
    for mi, m in enumerate(g["meshes"]):
        for pi, p in enumerate(m["primitives"]):
            if not p.get("targets"):
                continue
            n = g["accessors"][p["attributes"]["POSITION"]]["count"]
            order = _indices(g, buf, p["indices"]) if "indices" in p else np.arange(n)
            pd = np.stack([_accessor(g, buf, t["POSITION"])[order] for t in p["targets"]])
            nd = np.stack([_accessor(g, buf, t["NORMAL"])[order] for t in p["targets"]]) if all("NORMAL" in t for t in p["targets"]) else None
            prims.append({"mesh": mi, "primitive": pi, "position_deltas": pd, "normal_deltas": nd})
            defaults[mi] = np.asarray(m.get("weights", [0.0] * len(p["targets"])), dtype=F32)
    for an in g.get("animations", []):
        for ci, ch in enumerate(an["channels"]):
            if ch["target"]["path"] != "weights":
                continue
            mesh = g["nodes"][ch["target"]["node"]]["mesh"]
            smp = an["samplers"][ci]  # the sampler is picked by channel index, as for the other paths
            t = _accessor(g, buf, smp["input"]).reshape(-1)
            K = len(defaults[mesh])
            tracks.append({"mesh": mesh, "times": t, "values": _accessor(g, buf, smp["output"]).reshape(-1, K)})
    return {"primitives": prims, "defaults": defaults, "tracks": tracks}


def eval_weight_track(defaults, times, values, time):
    """The Track<> rule of host/scene.hpp on a weight track whose key 0 is the mesh's defaults at time 0: linear, component-wise, in fp32;
    a time before the first glTF key (but >= 0) and a time at or past the last key both give the LAST key (the reference's quirk)."""
    ts = np.concatenate([[F32(0)], np.asarray(times, dtype=F32)]).astype(F32)
    vs = np.concatenate([np.asarray(defaults, dtype=F32)[None], np.asarray(values, dtype=F32)]).astype(F32)
    time = F32(time)
    if len(ts) == 1 or time < 0:
        return vs[0]
    nxt = int(np.searchsorted(ts, time, side="right"))
    if nxt == 0 or nxt >= len(ts):
        return vs[-1]
    k = nxt - 1
    w = (time - ts[k]) / (ts[k + 1] - ts[k])
    return vs[k] * (F32(1.0) - w) + vs[k + 1] * w
