"""The build options a commit compares (hjr_prepare_transforms: lds_bvh, lds_stack16, bvh_width, leaf_max, bvh_refine, device_bvh,
device_bvh_opt, device_bvh_instances, device_bvh_graft), one context, the same transforms throughout.

The probe is the progressive-frame session: a commit that keeps the frame data lets an open frame's next pass in, a
commit that replaces it has the pass refused with HJR_ERR_STATE.  A commit of the same transforms keeps the frame data exactly while
none of the nine options changed; whatever was built instead renders the oracle's frame bit for bit.
"""
import ctypes as C

import numpy as np
import pytest

import oracle_binding as ob
from scene_util import Cornell, hjr

pytestmark = pytest.mark.gpu
W = H = SPP = 16  # granule 8: the passes [0, 8) and [8, 16)
ERR_STATE = -5
REFUSAL = "the frame data changed since the frame's first pass"
ALL = ("lds_bvh", "lds_stack16", "bvh_width", "leaf_max", "bvh_refine", "device_bvh", "device_bvh_opt", "device_bvh_instances", "device_bvh_graft",
       "force_rebuild")
DEVICE = {"device_bvh": 1, "lds_bvh": 0, "bvh_width": 4}  # what the device options are set on top of
# key field: (options of the frame data the frame starts on, the one option changed under it)
FIELDS = {
    "allow_lds": ({}, ("lds_bvh", 0)),
    "prefer_stack16": ({}, ("lds_stack16", 1)),
    "bvh_width": ({}, ("bvh_width", 4)),
    "leaf_max": ({}, ("leaf_max", 3)),
    "refine": ({}, ("bvh_refine", 1)),
    "device": ({"lds_bvh": 0, "bvh_width": 4}, ("device_bvh", 1)),
    "opt_rounds": (DEVICE, ("device_bvh_opt", 1)),
    "instances": (DEVICE, ("device_bvh_instances", 1)),
    "graft": (dict(DEVICE, device_bvh_instances=1), ("device_bvh_graft", 1)),
}


@pytest.fixture(scope="module")
def cornell():
    return Cornell()


@pytest.fixture(scope="module")
def dev(cornell):
    return cornell.device()


@pytest.fixture(scope="module")
def oracle_frame(cornell):
    return ob.OracleScene(cornell.arrays, ob.MATH_PORTABLE).render(cornell.oracle_params(W, H, SPP))[:3]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def commit(dev, cornell):
    dev.set_transforms(cornell.arrays["transforms"], cornell.arrays["inv_transforms"])


def render_pass(dev, cornell, begin, end):
    """(status, error text) of hjr_render on the sample pass [begin, end)."""
    p = cornell.hjr_params(W, H, SPP)
    p.sample_begin, p.sample_end = begin, end
    out = [np.zeros((H, W, 4), np.float32) for _ in range(3)]
    rc = hjr.lib().hjr_render(dev._h, C.byref(p), *[a.ctypes.data for a in out])
    return rc, hjr.lib().hjr_last_error().decode()


def open_frame(dev, cornell, options):
    """Every build option back to its default, then `options`; the frame data committed under them; the frame's first pass rendered."""
    for k in ALL:
        dev.set_option(k, options.get(k, -1))
    commit(dev, cornell)
    assert render_pass(dev, cornell, 0, 8)[0] == 0, hjr.lib().hjr_last_error()


def assert_refused_then_oracle(dev, cornell, oracle_frame, what):
    rc, msg = render_pass(dev, cornell, 8, 16)
    assert rc == ERR_STATE, (what, rc, msg)
    assert REFUSAL in msg, (what, msg)
    got = dev.render(cornell.hjr_params(W, H, SPP))
    for name, g, w in zip(("color", "albedo", "normal"), got, oracle_frame):
        same = bits(g) == bits(w)
        assert same.all(), "%s, %s: %d of %d values differ from the oracle" % (what, name, int((~same).sum()), same.size)


def test_commit_with_no_option_changed_keeps_the_frame(dev, cornell):
    """The control: the same transforms committed again under the same options, and the frame's second pass is accepted."""
    for options in ({}, DEVICE):
        open_frame(dev, cornell, options)
        commit(dev, cornell)
        rc, msg = render_pass(dev, cornell, 8, 16)
        assert rc == 0, (options, msg)


@pytest.mark.parametrize("field", list(FIELDS))
def test_one_changed_key_field_replaces_the_frame_data(dev, cornell, oracle_frame, field):
    base, (key, value) = FIELDS[field]
    open_frame(dev, cornell, base)
    assert base.get(key, -1) != value
    dev.set_option(key, value)
    commit(dev, cornell)
    assert_refused_then_oracle(dev, cornell, oracle_frame, "%s: \"%s\" %d" % (field, key, value))


def test_force_rebuild_replaces_the_frame_data(dev, cornell, oracle_frame):
    open_frame(dev, cornell, {})
    dev.set_option("force_rebuild", 1)
    commit(dev, cornell)
    assert_refused_then_oracle(dev, cornell, oracle_frame, "force_rebuild 1")
    dev.set_option("force_rebuild", -1)
