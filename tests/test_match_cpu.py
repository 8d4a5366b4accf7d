"""CPU tests for ba_match_descriptors: the pinned arithmetic (csrc/ba_match.h)
and the host packer run as a stand-alone host program under ASan + UBSan and
equal the numpy float32 restatement (tests/match_ref.py) bit for bit, which
also validates the restatement's fmaf emulation; the float32 matcher equals the
float64 brute-force one on scenes whose margins allow it; defaults, argument
errors and the ctypes mirrors are checked without a device.  No GPU."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import match_ref as R
from bundleadjustment_amd import _native as N
from bundleadjustment_amd.problem import MATCH_DTYPE, MATCH_KNN_DTYPE, pack_match_batch
from conftest import ROOT

HEADER = ROOT / "include" / "ba_hip.h"
F32 = np.float32


def hexbits(a) -> str:
    return " ".join(f"{v:08x}" for v in np.ascontiguousarray(a, F32).reshape(-1).view(np.uint32).tolist())


def case_text(sets, pairs, ratio=0.7, unique=1, max_distance=np.inf, row_ref=None, ref_desc=None, dim=None,
              set_offset=None) -> str:
    mb = pack_match_batch(sets, pairs, row_ref, ref_desc, dim=dim)
    off = mb.set_offset if set_offset is None else np.asarray(set_offset, np.int32)
    have_ref = mb.row_ref is not None
    n_ref = 0 if mb.ref_desc is None else mb.ref_desc.shape[0]
    lines = [f"{mb.dim} {off.size - 1} {mb.pairs.shape[0]} {n_ref} {int(have_ref)} {mb.desc.shape[0]} {hexbits([ratio])} {unique} "
             f"{hexbits([max_distance])}",
             " ".join(str(v) for v in off.tolist()),
             " ".join(f"{q} {t}" for q, t in mb.pairs.tolist()),
             hexbits(mb.desc)]
    if have_ref:
        lines += [" ".join(str(v) for v in mb.row_ref.tolist()), hexbits(mb.ref_desc)]
    return "\n".join(lines) + "\n"


def f32_of(words):
    return np.array([int(w, 16) for w in words], np.uint32).view(F32)


def parse(out: list[str]):
    """The host program's output: (plan, [(d2, knn, matches) per pair])."""
    plan = [int(x) for x in out[0].split()[1:]]
    pos, pairs = 1, []
    while pos < len(out):
        _, _i, nq, nt, nm = out[pos].split()
        nq, nt, nm = int(nq), int(nt), int(nm)
        pos += 1
        d2 = np.array([f32_of(out[pos + q].split()) for q in range(nq)], F32).reshape(nq, nt)
        pos += nq
        knn = np.zeros(nq, R.KNN_DTYPE)
        for q in range(nq):
            a, b, c, d = out[pos + q].split()
            knn[q] = (int(a), int(b), f32_of([c])[0], f32_of([d])[0])
        pos += nq
        m = np.zeros(nm, R.MATCH_DTYPE)
        for k in range(nm):
            a, b, c, d, e = out[pos + k].split()
            m[k] = (int(a), int(b), *f32_of([c, d, e]))
        pos += nm
        pairs.append((d2, knn, m))
    return plan, pairs


@pytest.fixture(scope="module")
def match_host(tmp_path_factory):
    exe = tmp_path_factory.mktemp("match_host") / "match_host"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fno-omit-frame-pointer",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    str(ROOT / "tests" / "cpp" / "match_host.cpp"), "-o", str(exe)], check=True)

    def run(text: str) -> list[str]:
        case = exe.parent / "case.txt"
        case.write_text(text)
        return subprocess.run([str(exe), str(case)], capture_output=True, text=True, check=True).stdout.splitlines()
    return run


def same_bits(a, b) -> bool:
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---------------------------------------------------------------------------
# the fmaf emulation
# ---------------------------------------------------------------------------
def test_fma32_rounds_once_where_rounding_twice_would_not():
    """(1 + 2^-23) 2^-12 * (1 - 2^-23) 2^-12 = 2^-24 - 2^-70; added to 1 + 2^-23
    the exact value lies just below the midpoint of 1 + 2^-23 and 1 + 2^-22.
    The float64 sum is that midpoint, and rounding it again would go to the
    even neighbour 1 + 2^-22."""
    a, b = F32((1 + 2.0 ** -23) * 2.0 ** -12), F32((1 - 2.0 ** -23) * 2.0 ** -12)
    c = F32(1 + 2.0 ** -23)
    assert F32(np.float64(a) * np.float64(b) + np.float64(c)) == F32(1 + 2.0 ** -22)      # the naive emulation
    assert R.fma32(a, b, c) == c and R.fma32(-a, b, -c) == -c
    assert R.fma32(F32(3), F32(5), F32(7)) == F32(22)
    # a true tie goes to even: 1 + 2^-24 exactly
    assert R.fma32(F32(2.0 ** -12), F32(2.0 ** -12), F32(1)) == F32(1)
    assert R.fma32(F32(2.0 ** -12), F32(2.0 ** -12), c) == F32(1 + 2.0 ** -22)


# ---------------------------------------------------------------------------
# the device's text as a host program under ASan + UBSan
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.CPU_SHAPES)
def test_host_program_equals_the_float32_restatement(match_host, shape):
    sc = R.scene(*shape)
    d2 = R.scene_d2_32(*shape)
    first = True
    for ratio, unique, maxd in ((0.7, 1, np.inf), (0.7, 0, np.inf), (0.9, 1, np.inf), (0.9, 0, 0.25)):
        plan, (got,) = parse(match_host(case_text([sc.Q, sc.T], [(0, 1)], ratio, unique, maxd, [sc.row_ref, None],
                                                  sc.ref_desc)))
        knn, m = R.match32(sc.Q, sc.T, ratio, unique, maxd, sc.row_ref, sc.ref_desc, d2=d2)
        if first:
            assert same_bits(got[0], d2), "d2"
            assert same_bits(got[1], knn), "2-NN"
            first = False
        assert same_bits(got[2], m), (ratio, unique, maxd)
        assert plan[2:5] == [shape[0], shape[1], min(shape[:2]) if unique else shape[0]]
    # the scene does what it was built for
    _, m = R.match32(sc.Q, sc.T, 0.7, 0, np.inf, sc.row_ref, sc.ref_desc, d2=d2)
    if shape[0] >= 63:
        assert m.size - np.unique(m["train"]).size == 3 and np.any(m["ref_distance"] >= 0)


def test_host_program_batch_shares_sets_and_keeps_empty_ones(match_host):
    """One batch: a set in several pairs, both directions, empty sets.  Each pair equals its own restatement."""
    a, b, c = R.scene(63, 65, 64), R.scene(65, 63, 64), R.scene(2, 2, 64)
    empty = np.zeros((0, 64), F32)
    sets = [a.Q, a.T, empty, b.T, c.Q]
    pairs = [(0, 1), (1, 0), (0, 3), (2, 1), (0, 2), (4, 4), (2, 2)]
    plan, got = parse(match_host(case_text(sets, pairs)))
    assert len(got) == len(pairs)
    for (q, t), (d2, knn, m) in zip(pairs, got):
        wk, wm = R.match32(sets[q], sets[t])
        assert same_bits(knn, wk) and same_bits(m, wm), (q, t)
    nq = [sets[q].shape[0] for q, _ in pairs]
    nt = [sets[t].shape[0] for _, t in pairs]
    assert plan[2:5] == [sum(nq), sum(nt), sum(min(x, y) for x, y in zip(nq, nt))]
    # a set against itself: every row finds itself at distance exactly 0
    self_knn = got[5][1]
    assert np.array_equal(self_knn["idx0"], [0, 1]) and np.all(self_knn["d2_0"] == 0)


def test_host_program_splits_a_long_train_set_into_chunks(match_host):
    """A single pair of 130 x 257 offers few query tiles: the plan deals the
    train rows to several chunks, and the merged lists equal the unsplit ones."""
    sc = R.scene(130, 257, 128)
    plan, (got,) = parse(match_host(case_text([sc.Q, sc.T], [(0, 1)])))
    chunks, chunk_rows = plan[:2]
    assert chunks == 3 and chunk_rows == 128 and chunk_rows % 64 == 0 and chunks * chunk_rows >= 257
    assert same_bits(got[1], R.match32(sc.Q, sc.T, d2=R.scene_d2_32(130, 257, 128))[0])


def test_host_program_tie_goes_to_the_lower_train_index(match_host):
    Q, T, t, copy = R.tie_scene()
    _, (got,) = parse(match_host(case_text([Q, T], [(0, 1)], unique=0)))
    d2, knn, m = got
    assert np.array_equal(d2[:, t].view(np.uint32), d2[:, copy].view(np.uint32))
    hit = knn["idx0"] == t
    assert hit.any() and not np.any(knn["idx0"] == copy)
    assert np.all(knn["idx1"][hit] == copy) and np.all(knn["d2_1"][hit] == knn["d2_0"][hit])
    assert not np.isin(np.nonzero(hit)[0], m["query"]).any()        # ratio 1 is rejected


@pytest.mark.parametrize("what,kw", [
    ("dim", dict(dim=32)),
    ("decreases", dict(set_offset=[0, 5, 3])),
    ("[0] != 0", dict(set_offset=[1, 5, 10])),
    ("out of range", dict(pairs=[(0, 2)])),
    ("out of range", dict(pairs=[(-1, 0)])),
    ("row_ref", dict(row_ref=[np.array([0, 1, 2, 3, 7]), None])),
    ("ratio", dict(ratio=-0.5)),
    ("ratio", dict(ratio=np.nan)),
    ("max_distance", dict(max_distance=np.nan)),
    ("unique", dict(unique=2)),
])
def test_host_program_checker_refuses(match_host, what, kw):
    dim = kw.pop("dim", 64)
    rng = np.random.default_rng(3)
    sets = [R.unit_rows(rng, 5, dim), R.unit_rows(rng, 5, dim)]
    args = dict(pairs=[(0, 1)], row_ref=[np.array([0, 1, -1, 2, 3]), None], ref_desc=R.unit_rows(rng, 4, dim))
    args.update(kw)
    out = match_host(case_text(sets, **args))
    assert len(out) == 1 and out[0].startswith("invalid match_host: ") and what in out[0], out


# ---------------------------------------------------------------------------
# float32 against float64
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.CPU_SHAPES)
def test_float32_matcher_equals_the_float64_one(shape):
    sc = R.scene(*shape)
    nq, nt, dim = shape
    bound = R.d2_bound(dim)
    assert abs(bound - {64: 1.6e-5, 128: 3.1e-5}[dim]) < 0.1e-5
    # ---- the scene: unit rows at full precision, margins that float32 cannot cross
    for X in (sc.Q, sc.T):
        assert np.max(np.abs(np.linalg.norm(X.astype(np.float64), axis=1) - 1.0)) < 1e-6
        assert np.any(np.round(X.astype(np.float64) * 4096) != X.astype(np.float64) * 4096)
    gap, margin, collisions = R.scene_margins(sc)
    print(f"{shape}: smallest gap {gap:.3g} (needs > {2 * bound:.3g}), ratio margin {margin:.3g}, "
          f"collisions {collisions}")
    assert gap > 2 * bound and margin > 1e-3
    if min(nq, nt) >= 63:
        assert collisions == 3
    # ---- float32 == float64
    d2 = R.scene_d2_32(*shape)
    err = float(np.max(np.abs(d2.astype(np.float64) - R.d2_64(sc.Q, sc.T))))
    print(f"{shape}: max |d2_f32 - d2_f64| = {err:.3g} (bound {bound:.3g})")
    assert err <= bound
    for unique in (1, 0):
        knn32, m = R.match32(sc.Q, sc.T, 0.7, unique, d2=d2)
        knn64, srt, q, t = R.match64(sc.Q, sc.T, 0.7, unique)
        assert np.array_equal(knn32["idx0"], knn64["idx0"]) and np.array_equal(knn32["idx1"], knn64["idx1"])
        assert np.array_equal(m["query"], q) and np.array_equal(m["train"], t)
        assert np.max(np.abs(knn32["d2_0"].astype(np.float64) - srt[:, 0])) <= bound
        assert np.max(np.abs(knn32["d2_1"].astype(np.float64) - srt[:, 1])) <= bound
        # the matches are the planted ones (a near-duplicate query competes for its source's train row)
        for qq, tt in zip(q.tolist(), t.tolist()):
            src = dict(sc.dup).get(qq, qq)
            assert sc.truth.get(src) == tt, (qq, tt)
    if shape == (1, 5, 64):
        assert R.match32(sc.Q, sc.T, d2=d2)[1].size == 0


# ---------------------------------------------------------------------------
# ABI
# ---------------------------------------------------------------------------
STRUCTS = {"ba_match_batch": N.ba_match_batch, "ba_match_options": N.ba_match_options, "ba_match": N.ba_match,
           "ba_match_neighbors": N.ba_match_neighbors}


def test_ctypes_layout_of_the_match_structs_matches_c(tmp_path):
    body = "".join(f'  printf("{t} %zu\\n", sizeof({t}));\n' +
                   "".join(f'  printf("{t}.{f} %zu\\n", offsetof({t}, {f}));\n' for f, _ in cls._fields_)
                   for t, cls in STRUCTS.items())
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ba_hip.h"\nint main(void) {\n' + body +
                   '  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(lines) == len(STRUCTS) + sum(len(c._fields_) for c in STRUCTS.values())
    for line in lines:
        k, v = line.split()
        if "." in k:
            t, f = k.split(".")
            assert getattr(STRUCTS[t], f).offset == int(v), k
        else:
            assert C.sizeof(STRUCTS[k]) == int(v), k
    assert MATCH_DTYPE.itemsize == C.sizeof(N.ba_match) and MATCH_KNN_DTYPE.itemsize == C.sizeof(N.ba_match_neighbors)
    assert MATCH_DTYPE == R.MATCH_DTYPE and MATCH_KNN_DTYPE == R.KNN_DTYPE


def test_header_names_the_match_symbols():
    txt = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    fns = set(re.findall(r"\b(ba_[a-z0-9_]+)\s*\(", txt))
    assert {"ba_match_defaults", "ba_match_descriptors", "ba_match_times", "ba_match_knn"} <= fns
    assert re.search(r"#define\s+BA_ABI_VERSION\s+2\b", txt)


def test_match_entry_points_and_defaults_without_a_device():
    lib = N.load_library()
    p = N.ba_match_options()
    lib.ba_match_defaults(C.byref(p))
    assert (p.ratio, p.unique, p.max_distance, p.reserved) == (float(F32(0.7)), 1, np.inf, 0)
    lib.ba_match_defaults(None)
    assert lib.ba_match_descriptors(None, None, None, None, None) == 1   # BA_ERR_INVALID_ARGUMENT
    assert lib.ba_match_knn(None, None, 0, None) == 1
    assert lib.ba_match_times(None, None, 0) == -1
    assert lib.ba_abi_version() == 2


def test_pack_match_batch_layout():
    rng = np.random.default_rng(0)
    sets = [R.unit_rows(rng, 3, 64), np.zeros((0, 64), F32), R.unit_rows(rng, 2, 64)]
    mb = pack_match_batch(sets, [(0, 2), (2, 0)], row_ref=[[0, -1, 1], None, None], ref_desc=R.unit_rows(rng, 2, 64))
    assert mb.dim == 64 and mb.set_offset.tolist() == [0, 3, 3, 5] and mb.desc.shape == (5, 64)
    assert mb.desc.dtype == F32 and mb.desc.flags.c_contiguous and np.array_equal(mb.desc[3:], sets[2])
    assert mb.row_ref.tolist() == [0, -1, 1, -1, -1] and mb.pairs.tolist() == [[0, 2], [2, 0]]
    assert pack_match_batch([np.zeros((0, 128))], np.zeros((0, 2)), dim=128).desc.shape == (0, 128)
    with pytest.raises(ValueError):
        pack_match_batch([R.unit_rows(rng, 2, 64), R.unit_rows(rng, 2, 128)], [(0, 1)])
