"""Option "item_chunks": the megakernel's work items as groups of 1, 2, 4 or 8 consecutive chunks of a pixel.

Grouping is scheduling only: a lane that finishes a chunk writes that chunk's sum to the chunk's own slot and goes on with the pixel's next
chunk instead of fetching a new item, so every frame must stay the oracle's frame bit for bit and every ray / hit / sample counter must
stay what single-chunk items give.  Bundled Cornell scene at 24x16 (3x2 tiles) and the ragged 21x13 (edge tiles in both directions), 32 spp
(4 chunks of 8: groups of 1, 2 and 4) and 24 spp (3 chunks: every request falls back to 1): the smallest sizes at which a chunk boundary
inside an item, a ragged edge tile, an odd chunk count and a shard all occur."""
import ctypes as C

import numpy as np
import pytest

import oracle_binding as ob
from scene_util import Cornell, hjr
from test_gpu_parity import assert_bitexact

pytestmark = pytest.mark.gpu

COUNTERS = ("samples", "closest_rays", "shadow_rays", "box_tests_closest", "tri_tests_closest", "box_tests_shadow", "tri_tests_shadow",
            "shaded_hits", "light_samples", "nan_samples")


@pytest.fixture(scope="module")
def cornell():
    return Cornell()


@pytest.fixture(scope="module")
def dev(cornell):
    d = cornell.device({"pipeline": 1})  # the megakernel, whatever the integrator
    yield d
    d.close()


@pytest.fixture(scope="module")
def dev_memory(cornell):
    d = cornell.device({"pipeline": 1, "lds_bvh": 0})  # BVH4 read from memory (hjr_stats.lds_mode 0)
    yield d
    d.close()


_oracle = {}


def oracle_frame(cornell, w, h, spp, integrator=hjr.INTEGRATOR_NEE):
    """(colour, albedo, normal) of the CPU oracle, rendered once per configuration and shared by the tests."""
    k = (w, h, spp, integrator)
    if k not in _oracle:
        oc, oa, on, st = ob.OracleScene(cornell.arrays, ob.MATH_PORTABLE).render(cornell.oracle_params(w, h, spp, integrator=integrator))
        assert st["nan_samples"] == 0
        for a in (oc, oa, on):
            a.setflags(write=False)
        _oracle[k] = (oc, oa, on)
    return _oracle[k]


def effective(request, chunks):
    """hjr_item_chunks (csrc/hjr_layout.h): the largest power of two that is no larger than the request and divides the launch's chunks."""
    r = 1
    while r * 2 <= request and chunks % (r * 2) == 0:
        r *= 2
    return r


def counters(d):
    st = d.stats()
    return {k: st[k] for k in COUNTERS}


def render_checked(d, cornell, w, h, spp, item_chunks, integrator=hjr.INTEGRATOR_NEE):
    """Frames with `item_chunks` set (all AOVs, then colour only) against the oracle; returns the counters of a counting launch."""
    oc, oa, on = oracle_frame(cornell, w, h, spp, integrator)
    d.set_option("item_chunks", item_chunks)
    try:
        what = "item_chunks %d, %dx%dx%d, integrator %d" % (item_chunks, w, h, spp, integrator)
        used = effective(item_chunks, (spp + 7) // 8)  # what hjr_stats.item_chunks must report for every launch below
        color, albedo, normal = d.render(cornell.hjr_params(w, h, spp, integrator=integrator))
        assert d.stats()["pipeline"] == 0 and d.stats()["item_chunks"] == used, d.stats()
        assert_bitexact(color, oc, "aov_color (" + what + ")")
        assert_bitexact(albedo, oa, "aov_albedo (" + what + ")")
        assert_bitexact(normal, on, "aov_normal (" + what + ")")
        lean, _, _ = d.render(cornell.hjr_params(w, h, spp, integrator=integrator), want_aovs=False)
        assert d.stats()["item_chunks"] == used
        assert_bitexact(lean, oc, "aov_color, colour-only kernel (" + what + ")")
        counted, _, _ = d.render(cornell.hjr_params(w, h, spp, integrator=integrator, flags=hjr.FLAG_STATS), want_aovs=False)
        assert d.stats()["item_chunks"] == used
        assert_bitexact(counted, oc, "aov_color, counting kernel (" + what + ")")
        return counters(d)
    finally:
        d.set_option("item_chunks", -1)


_single = {}


def single_chunk_counters(d, cornell, key, *a, **kw):
    if key not in _single:
        _single[key] = render_checked(d, cornell, *a, item_chunks=1, **kw)
    return _single[key]


@pytest.mark.parametrize("item_chunks", [1, 2, 4])
@pytest.mark.parametrize("spp", [32, 24])
@pytest.mark.parametrize("w,h", [(24, 16), (21, 13)])
def test_frames_and_counters_do_not_depend_on_item_chunks(cornell, dev, w, h, spp, item_chunks):
    ref = single_chunk_counters(dev, cornell, ("nee", w, h, spp), w, h, spp)
    assert ref["samples"] == w * h * spp
    got = render_checked(dev, cornell, w, h, spp, item_chunks)
    assert got == ref


@pytest.mark.parametrize("item_chunks", [2, 4])
def test_pathtrace(cornell, dev, item_chunks):
    ref = single_chunk_counters(dev, cornell, ("pt",), 24, 16, 32, integrator=hjr.INTEGRATOR_PT)
    assert render_checked(dev, cornell, 24, 16, 32, item_chunks, integrator=hjr.INTEGRATOR_PT) == ref


@pytest.mark.parametrize("item_chunks", [2, 4])
def test_memory_layout(cornell, dev_memory, item_chunks):
    ref = single_chunk_counters(dev_memory, cornell, ("mem",), 24, 16, 32)
    assert dev_memory.stats()["lds_mode"] == 0
    assert render_checked(dev_memory, cornell, 24, 16, 32, item_chunks) == ref


def render_raw(d, p, shape, want_aovs=True):
    out = [np.zeros(shape, np.float32) for _ in range(3 if want_aovs else 1)]
    rc = hjr.lib().hjr_render(d._h, C.byref(p), out[0].ctypes.data, out[1].ctypes.data if want_aovs else None, out[2].ctypes.data if want_aovs else None)
    assert rc == 0, hjr.lib().hjr_last_error()
    return out


def test_rank_of_a_shard_with_packed_tiles(cornell, dev):
    """Rank 1 of 2, HJR_FLAG_PACKED, explicit item_chunks 2 (a shard's default is 1): its tiles of the oracle's frame, its counters."""
    w, h, spp, rank, world = 24, 16, 32, 1, 2
    ora = oracle_frame(cornell, w, h, spp)
    n = hjr.owned_tiles(w, h, rank, world)
    mask = hjr.owned_tile_mask(w, h, rank, world)
    result = {}
    for item_chunks in (1, 2):
        dev.set_option("item_chunks", item_chunks)
        try:
            out = render_raw(dev, cornell.hjr_params(w, h, spp, rank=rank, world_size=world, flags=hjr.FLAG_PACKED), (n, 64, 4))
            assert dev.stats()["item_chunks"] == item_chunks
            for a, o, name in zip(out, ora, ("color", "albedo", "normal")):
                frame = np.zeros((h, w, 4), np.float32)
                hjr.unpack_tiles(a, frame, rank, world)
                assert_bitexact(frame[mask][None], o[mask][None], "aov_%s of rank %d / %d, item_chunks %d" % (name, rank, world, item_chunks))
            render_raw(dev, cornell.hjr_params(w, h, spp, rank=rank, world_size=world, flags=hjr.FLAG_PACKED | hjr.FLAG_STATS), (n, 64, 4), want_aovs=False)
            assert dev.stats()["item_chunks"] == item_chunks
            result[item_chunks] = counters(dev)
        finally:
            dev.set_option("item_chunks", -1)
    assert result[1]["samples"] == int(mask.sum()) * spp
    assert result[2] == result[1]


@pytest.mark.parametrize("split", [8, 16])
@pytest.mark.parametrize("item_chunks", [1, 2, 4])
def test_two_sample_passes(cornell, dev, item_chunks, split):
    """[0, 8) and [8, 32): one chunk, then three chunks starting at chunk 1 (every request falls back to single chunks there).
    [0, 16) and [16, 32): two chunks each, the second pass starting at chunk 2, so pairs run with chunk0 != 0 (the item rule counts chunks
    from chunk0, the chunk-sum pointers of the pass are moved back by chunk0 chunks and the item word moves on inside an item)."""
    w, h, spp = 24, 16, 32
    oc, oa, on = oracle_frame(cornell, w, h, spp)
    dev.set_option("item_chunks", item_chunks)
    try:
        total = dict.fromkeys(COUNTERS, 0)
        for flags in (0, hjr.FLAG_STATS):
            for b, e in ((0, split), (split, 32)):
                color, albedo, normal = dev.render(cornell.hjr_params(w, h, spp, flags=flags, sample_begin=b, sample_end=e))
                assert dev.stats()["item_chunks"] == effective(item_chunks, (e - b) // 8)
                if flags:
                    for k, v in counters(dev).items():
                        total[k] += v
            assert_bitexact(color, oc, "aov_color after two passes, item_chunks %d, flags %d" % (item_chunks, flags))
            assert_bitexact(albedo, oa, "aov_albedo after two passes")
            assert_bitexact(normal, on, "aov_normal after two passes")
    finally:
        dev.set_option("item_chunks", -1)
    assert total == single_chunk_counters(dev, cornell, ("nee", w, h, spp), w, h, spp)


def test_default_selection(cornell, dev):
    """With the option unset the launch decides (hjr_render.hip::launch_render): pairs for a single-GPU launch of at least 192 single-chunk
    items per lane of the grid — the headline shape, 1080p x 256 spp —, single chunks for a short launch, a rank of a shard and a counting
    launch.  The headline frame with the default is the frame of single chunks, bit for bit."""
    w, h = 1920, 1080
    assert dev.get_option("item_chunks") == -1
    paired, _, _ = dev.render(cornell.hjr_params(w, h, 256), want_aovs=False)
    assert dev.stats()["item_chunks"] == 2, dev.stats()
    dev.set_option("item_chunks", 1)
    try:
        single, _, _ = dev.render(cornell.hjr_params(w, h, 256), want_aovs=False)
        assert dev.stats()["item_chunks"] == 1
    finally:
        dev.set_option("item_chunks", -1)
    assert np.array_equal(paired.view(np.uint32), single.view(np.uint32))
    dev.render(cornell.hjr_params(w, h, 64), want_aovs=False)  # 63 items per lane
    assert dev.stats()["item_chunks"] == 1
    dev.render(cornell.hjr_params(64, 64, 256, flags=hjr.FLAG_STATS), want_aovs=False)
    assert dev.stats()["item_chunks"] == 1
    n = hjr.owned_tiles(w, h, 0, 2)
    render_raw(dev, cornell.hjr_params(w, h, 256, rank=0, world_size=2, flags=hjr.FLAG_PACKED), (n, 64, 4), want_aovs=False)
    assert dev.stats()["item_chunks"] == 1


def test_option_values(dev):
    for bad in (0, 3, 5, 6, 7, 16):
        with pytest.raises(hjr.HjrError):
            dev.set_option("item_chunks", bad)
    for good in (1, 2, 4, 8, -1):
        dev.set_option("item_chunks", good)
        assert dev.get_option("item_chunks") == good
