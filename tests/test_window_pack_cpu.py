"""CPU tests of the batched small-window interface: pack_window_batch (pure
numpy) and the ctypes mirror of ba_window_batch.  No compute calls."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from bundleadjustment_amd import Problem, WindowBatch, make_synthetic, pack_window_batch
from bundleadjustment_amd import _native as N
from bundleadjustment_amd.problem import fix_camera
from conftest import ROOT

ARRAYS = {"cams": (np.float64, (6,)), "cam_fixed": (np.uint8, ()), "cam_fixed_extr": (np.float32, (16,)),
          "K": (np.float32, (9,)), "pts": (np.float64, (3,)), "pt_fixed": (np.uint8, ()),
          "obs_cam": (np.int32, ()), "obs_pt": (np.int32, ()), "obs_uv": (np.float32, (2,))}
OWNER = {"cams": "cam", "cam_fixed": "cam", "cam_fixed_extr": "cam", "K": "cam", "pts": "pt", "pt_fixed": "pt",
         "obs_cam": "obs", "obs_pt": "obs", "obs_uv": "obs"}


def ragged():
    a = fix_camera(fix_camera(make_synthetic(5, 40, 3, seed=0xBA5E0101), 1), 0)
    b = make_synthetic(3, 7, 2, seed=0xBA5E0102, intr="replica")
    b.pt_fixed = np.zeros(b.n_pts, np.uint8)
    b.pt_fixed[::2] = 1
    # bare container: no fixed flags, no extrinsics, non-contiguous / wide dtypes
    c = Problem(cams=np.arange(12, dtype=np.float64).reshape(2, 6)[::-1], K=np.ones((2, 9), np.float64),
                pts=np.zeros((1, 3), np.float32), obs_cam=np.array([1, 0, 1], np.int64),
                obs_pt=np.array([0, 0, 0], np.int64), obs_uv=np.ones((3, 2), np.float64))
    return [a, b, c]


def test_pack_offsets_dtypes_and_round_trip():
    ps = ragged()
    b = pack_window_batch(ps)
    assert isinstance(b, WindowBatch) and b.n_problems == 3
    for name, counts in (("cam_offset", [p.n_cams for p in ps]), ("pt_offset", [p.n_pts for p in ps]),
                         ("obs_offset", [p.n_obs for p in ps])):
        off = getattr(b, name)
        assert off.dtype == np.int32 and off.flags.c_contiguous and off.shape == (4,)
        assert off[0] == 0 and list(np.diff(off)) == counts
    for name, (dt, tail) in ARRAYS.items():
        a = getattr(b, name)
        total = int(getattr(b, OWNER[name] + "_offset")[-1])
        assert a.dtype == dt and a.flags.c_contiguous and a.shape == (total,) + tail, name
    assert b.huber_a == ps[0].huber_a
    # slicing gives back each problem; indices stay local
    for i, p in enumerate(ps):
        q = p.normalized()
        for name in ARRAYS:
            off = getattr(b, OWNER[name] + "_offset")
            got = getattr(b, name)[off[i]:off[i + 1]]
            want = getattr(q, name)
            if want is None:   # a missing flag / extrinsic array packs as zeros
                assert not got.any(), (i, name)
            else:
                assert np.array_equal(got, want), (i, name)
        oc = b.obs_cam[b.obs_offset[i]:b.obs_offset[i + 1]]
        op = b.obs_pt[b.obs_offset[i]:b.obs_offset[i + 1]]
        assert oc.min() >= 0 and oc.max() < p.n_cams and op.min() >= 0 and op.max() < p.n_pts


def test_pack_empty_and_zero_observation_problem():
    e = pack_window_batch([])
    assert e.n_problems == 0 and e.cams.shape == (0, 6) and e.obs_uv.shape == (0, 2)
    p = make_synthetic(3, 5, 2, seed=0xBA5E0103)
    p.obs_cam, p.obs_pt, p.obs_uv = p.obs_cam[:0], p.obs_pt[:0], p.obs_uv[:0]
    b = pack_window_batch([p, p])
    assert list(b.obs_offset) == [0, 0, 0] and list(b.cam_offset) == [0, 3, 6]


def test_pack_refuses_mixed_huber():
    ps = ragged()
    ps[1].huber_a = 0.0
    with pytest.raises(ValueError, match="huber_a"):
        pack_window_batch(ps)


LAYOUT_C = r"""
#include <stdio.h>
#include <stddef.h>
#include "ba_hip.h"
#define F(f) printf("%s %zu\n", #f, offsetof(ba_window_batch, f));
int main(void) {
  printf("sizeof %zu\nmax_cams %d\nabi %d\n", sizeof(ba_window_batch), BA_WINDOW_MAX_CAMS, BA_ABI_VERSION);
  F(n_problems) F(reserved) F(cam_offset) F(pt_offset) F(obs_offset) F(cams) F(cam_fixed) F(cam_fixed_extr) F(K)
  F(pts) F(pt_fixed) F(obs_cam) F(obs_pt) F(obs_uv) F(huber_a)
  return 0;
}
"""


def test_window_batch_ctypes_layout_matches_c_compiler(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text(LAYOUT_C)
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    lines = [ln.split() for ln in subprocess.run([str(exe)], capture_output=True, text=True,
                                                 check=True).stdout.splitlines()]
    vals = {k: int(v) for k, v in lines}
    assert C.sizeof(N.ba_window_batch) == vals.pop("sizeof")
    assert N.BA_WINDOW_MAX_CAMS == vals.pop("max_cams") == 16
    assert N.BA_ABI_VERSION == vals.pop("abi") == 2
    # every field, in the header's order
    assert [f for f, _ in N.ba_window_batch._fields_] == [k for k, _ in lines[3:]]
    for f, off in vals.items():
        assert getattr(N.ba_window_batch, f).offset == off, f


def test_window_entry_points_are_bound():
    names = {name for name, _, _ in N.SIGNATURES}
    assert {"ba_solve_window_batch", "ba_get_window_iteration_log"} <= names
    lib = N.load_library()
    assert lib.ba_solve_window_batch(None, None, None, None, None, None) == 1
    assert lib.ba_get_window_iteration_log(None, 0, None, 0) < 0
