"""Resizing and compacting a kept map without a GPU: the restated move (tests/map_rehash_restatement.py) against the restated
builds and removals, the claims of the constructed inputs that tests/test_map_rehash_gpu.py relies on, the host-side
refusals of ``MapLocalizer.resize*`` / ``fit``, the argument checks of nsc_map_rehash_dist, the shape of its symbol and the
registers of its kernels."""
import ctypes as C

import numpy as np
import pytest

import map_insert_cases as IK
import map_insert_restatement as IR
import map_localize_cases as K
import map_localize_restatement as R
import map_rehash_restatement as HR
import map_replace_restatement as PR
import map_restatement as M
from test_map_insert_cpu import group, joined
from test_map_replace_cpu import state

FORMATS = [(np.float32, 3), (np.float32, 4), (np.float64, 3)]
SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8193]


@pytest.fixture(scope="module")
def lib():
    from neural_spectral_codec_amd import build, _lib
    build.build_hip()
    return _lib.lib()


def four_groups(dtype=np.float32, cols=3):
    g = IK.general_split(dtype, cols)
    return [group(g, [n]) for n in ("A", "B", "C_old", "C_new")]


def build_kept(parts, max_voxels, **kw):
    """the restated build over all parts -> its kept tensors on the host"""
    p, o, T = joined(parts)
    return HR.as_kept(R.build_dist(p, o, T, max_voxels=max_voxels, **kw), cursor=[len(p), len(o) - 1])


def assert_same_kept(got, want, what=""):
    """a restated move and a restated build agree by bits where a map is defined, and a lookup finds the same"""
    assert got["stats"].tolist() == want["stats"].tolist(), (what, got["stats"], want["stats"])
    n = int(want["stats"][1])
    for k in ("voxels", "info", "keys", "moments"):
        assert got[k][:n].tobytes() == want[k][:n].tobytes(), (what, k)
    assert got["cursor"].tolist() == want["cursor"].tolist() and got["place"] == want["place"], what


def mapping(k):
    """kept tensors and ``place`` -> {key: (count, the moments' bytes, the record's bytes)} of the voxels with a place"""
    return {key: (int(k["info"][p, 0]), k["moments"][p].tobytes(), k["voxels"][p].tobytes())
            for key, p in k["place"].items() if p >= 0}


# ---- 1. the restatement against the restated builds -------------------------------------------------------------------

@pytest.mark.parametrize("dtype,cols", FORMATS)
def test_restated_move_equals_the_restated_build_at_the_other_capacity(dtype, cols):
    parts = four_groups(dtype, cols)
    src = build_kept(parts, 512)
    found = int(src["stats"][0])
    assert found <= 512 and int(src["stats"][1]) == found                # equality with a build is claimed below
    for size in (2048, 512, found):
        out = HR.rehash(src, False, size)
        assert_same_kept(out, build_kept(parts, size), size)
        assert out["rehashed"].tolist() == [found, 0, 0, 0, 0, 0]
        assert out["new_place"].tolist() == list(range(found)) + [-1] * (512 - found)
        assert out["tile_base"].tolist() == [0, found]
    # too small: the build's overflow, while the keys fit into the slots
    size = (3 * found) // 5
    assert size < found <= 2 * size
    out = HR.rehash(src, False, size)
    assert_same_kept(out, build_kept(parts, size), "too small")
    assert out["rehashed"].tolist() == [found, 0, 0, 0, found - size, 0]
    assert found > 2 * (found // 3)
    out = HR.rehash(src, False, found // 3)
    assert out["place"] is None and out["rehashed"].tolist() == [found, 0, 0, 0, found - found // 3, found - 2 * (found // 3)]


@pytest.mark.parametrize("dtype,cols", FORMATS)
def test_restated_compaction_equals_the_restated_build_over_what_remains(dtype, cols):
    A, B, Co, Cn = parts = four_groups(dtype, cols)
    s = state(parts, 512)
    emptied_places = PR.remove(s, *Cn)[2] + PR.remove(s, *B)[2]
    src = HR.as_kept(IR.arrays(s))
    emptied, bad = HR.kinds(src)
    assert sorted(np.nonzero(emptied)[0].tolist()) == sorted(emptied_places) and len(emptied_places) > 10 and not bad.any()
    rest = R.build_dist(*joined([A, Co]), max_voxels=512)
    left = int(rest["voxels_found"])
    assert left == int(src["stats"][1]) - len(emptied_places) <= 512
    for size in (512, left):
        out = HR.rehash(src, False, size)
        assert mapping(out) == mapping(HR.as_kept(rest, cursor=[0, 0]))
        assert out["stats"].tolist() == [left, left] + src["stats"][2:].tolist()
        assert out["rehashed"].tolist() == [left, len(emptied_places), 0, 0, 0, 0]
        assert (np.diff(out["info"][:left, 1]) > 0).all()               # ascending first row survives
    kept_all = HR.rehash(src, True, 512)
    assert_same_kept(kept_all, src, "emptied voxels kept")
    assert kept_all["rehashed"].tolist() == [int(src["stats"][1]), 0, 0, 0, 0, 0]
    # C_new alone removed and a destination of three fifths of the build: too small, and the keys fit into the slots
    found = int(build_kept(parts, 512)["stats"][0])
    size = (3 * found) // 5
    s = state(parts, 512)
    gone = len(PR.remove(s, *Cn)[2])
    assert gone > 10 and size < found - gone <= 2 * size and found - gone <= 300
    out = HR.rehash(HR.as_kept(IR.arrays(s)), False, size)
    assert out["rehashed"].tolist() == [found - gone, gone, 0, 0, found - gone - size, 0]
    assert sorted(p for p in out["place"].values() if p >= 0) == list(range(size))
    # the sequence of the repeatability test stays inside its capacities
    assert int(build_kept([A, B, Co, Cn], 256)["stats"][0]) <= 256


# ---- 2. the claims of the other constructed inputs --------------------------------------------------------------------

def lattice_kept(n):
    """the kept integers of tests/test_map_rehash_gpu.py lattice_map(n): n voxels of one row, every third emptied"""
    cap = max(n, 1)
    info = np.zeros((cap, 4), np.int64)
    info[:n, 0] = np.arange(n) % 3 != 0
    info[:n, 1] = info[:n, 2] = info[:n, 3] = np.arange(n)
    gone = (n + 2) // 3
    return dict(voxels=np.zeros((cap, 16)), info=info, keys=np.arange(cap, dtype=np.int64) + 7,
                moments=np.zeros((cap, 9), np.int64), stats=np.array([n, n, n - gone, 0, 0, 0, 0], np.int64),
                cursor=np.array([n, n], np.int64)), gone


def test_the_sweep_of_sizes_reaches_every_boundary():
    """places that end one short of, at and one past a wave of 64, a sweep of 256 and a tile of 4096; two and three tiles,
    whose counts differ; lattice points of distinct voxels"""
    for unit in (64, 256, 4096):
        assert {unit - 1, unit, unit + 1} <= set(SIZES)
    i = np.arange(max(SIZES))
    vox = np.stack([i % 64, (i // 64) % 64, i // 4096], 1)
    assert len(np.unique(vox, axis=0)) == len(i)
    counts = {}
    for n in SIZES:
        k, gone = lattice_kept(n)
        out = HR.rehash(k, False, max(n - gone, 1))
        assert out["rehashed"].tolist() == [n - gone, gone, 0, 0, 0, 0] and out["stats"][:2].tolist() == [n - gone, n - gone]
        assert out["tile_base"].shape == (-(-max(n, 1) // 4096) + 1,) and out["tile_base"][-1] == n - gone
        assert out["info"][:n - gone, 1].tolist() == [r for r in range(n) if r % 3]
        counts[n] = np.diff(out["tile_base"]).tolist()
    assert counts[0] == [0] and counts[1] == [0] and counts[4097] == [2730, 1] and counts[8193] == [2730, 2731, 1]


def test_the_scene_and_the_twelve_voxels():
    s = K.scene()
    whole = set(M.build_map(s["points"], s["offsets"], s["poses"], voxel_size=1.0)["keys"].tolist())
    four = set(M.build_map(s["points"][:16000], s["offsets"][:5], s["poses"][:4], voxel_size=1.0)["keys"].tolist())
    assert len(whole) <= 8192 and four < whole                           # removing clouds 4 and 5 empties voxels
    # B removed twice from a map that holds A twice: five inconsistent voxels, none emptied
    A, B, vox = IK.twelve_voxels()
    st = state([A, A, B], 16)
    for _ in range(2):
        PR.remove(st, *B)
    k = HR.as_kept(IR.arrays(st))
    emptied, bad = HR.kinds(k)
    assert int(k["stats"][0]) == 12 and not emptied.any() and int(bad.sum()) == 5
    out = HR.rehash(k, False, 12)
    assert out["rehashed"].tolist() == [12, 0, 0, 5, 0, 0] and out["info"][:12, 0].tolist() == k["info"][:12, 0].tolist()
    # without moments the count alone decides: a count of 0 with a moment left is dropped as emptied
    k["info"][0, 0], k["moments"][0, 0] = 0, 3
    assert HR.rehash(k, False, 12)["rehashed"].tolist() == [12, 0, 0, 6, 0, 0]
    del k["moments"]
    assert HR.rehash(k, False, 12)["rehashed"].tolist() == [11, 1, 0, 5, 0, 0]


# ---- 3. refusals ------------------------------------------------------------------------------------------------------

def test_resize_refusals_on_the_host():
    import torch
    from neural_spectral_codec_amd import _lib
    from neural_spectral_codec_amd.retrieval import MapLocalizer
    m = MapLocalizer(insertable=True, max_voxels=16)
    for call in (lambda: m.resize_device(32), lambda: m.resize(32), lambda: m.fit(), lambda: m.resize_device()):
        with pytest.raises(_lib.NscError, match="build a map first"):
            call()
    m.voxels, m.capacity = torch.zeros(16, 16), 16                          # as if a map were there
    for size in (0, -1, _lib.MAP_MAX_VOXELS + 1):
        for call in (m.resize_device, m.resize):
            with pytest.raises(_lib.NscError, match="max_voxels must lie in"):
                call(size)
    for headroom in (0.5, float("nan"), float("inf"), -2.0):
        with pytest.raises(_lib.NscError, match="headroom must be finite and at least 1"):
            m.fit(headroom)


def test_abi_refusals_and_constants(lib):
    import os
    import re
    from neural_spectral_codec_amd import _lib
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "nsc.h")).read()
    for name, value in (("NSC_MAP_REHASH_LAUNCHES", _lib.MAP_REHASH_LAUNCHES), ("NSC_MAP_REHASH_STATS", _lib.MAP_REHASH_STATS)):
        assert int(re.search(rf"#define {name}\s+(\d+)", header).group(1)) == value, name
    assert len(_lib.MAP_REHASH_STAT_NAMES) == _lib.MAP_REHASH_STATS == 6 and _lib.MAP_REHASH_LAUNCHES == 4
    assert len(re.findall(r"#define NSC_MAP_REHASH_STAT_[A-Z_]+\s+\d", header)) == 6
    some = lambda n=64: (C.c_int64 * n)()
    src = dict(voxels=(C.c_double * 64)(), info=some(), keys=some(), moments=some(), stats=some(), cursor=some())
    dst = dict(new_voxels=(C.c_double * 64)(), new_index=(C.c_uint64 * 64)(), new_info=some(), new_keys=some(),
               new_moments=some(), new_stats=some(), new_cursor=some(), new_place=some(), tile_base=some(), rehashed=some())

    def call(max_voxels=4, new_max_voxels=4, **kw):
        a = dict(src, **dst)
        a.update(kw)
        return lib.nsc_map_rehash_dist(a["voxels"], a["info"], a["keys"], a["moments"], a["stats"], a["cursor"], max_voxels, 0,
                                       a["new_voxels"], a["new_index"], a["new_info"], a["new_keys"], a["new_moments"],
                                       a["new_stats"], a["new_cursor"], new_max_voxels, a["new_place"], a["tile_base"],
                                       a["rehashed"], None)
    # a null among the required pointers
    for name in ("voxels", "info", "keys", "stats", "new_voxels", "new_index", "new_info", "new_keys", "new_stats", "new_place",
                 "tile_base", "rehashed"):
        assert call(**{name: None}) == -1, name
    # sizes
    assert call(max_voxels=-1) == -1 and call(new_max_voxels=0) == -1 and call(new_max_voxels=-5) == -1
    assert call(max_voxels=_lib.MAP_MAX_VOXELS + 1) == -2 and call(new_max_voxels=_lib.MAP_MAX_VOXELS + 1) == -2
    # moments or cursor on one side only
    assert call(moments=None) == -1 and call(new_moments=None) == -1
    assert call(cursor=None) == -1 and call(new_cursor=None) == -1
    # a destination that is its source: the call is out of place
    for a, b in (("voxels", "new_voxels"), ("info", "new_info"), ("keys", "new_keys"), ("moments", "new_moments"),
                 ("stats", "new_stats"), ("cursor", "new_cursor")):
        assert call(**{b: src[a]}) == -1, a


def test_the_symbol_takes_no_workspace():
    """the entry points with a size_t argument stay the 28 of tests/workspace_contract.py; the arrays
    this call needs beyond the map are typed outputs"""
    import workspace_contract as W
    from neural_spectral_codec_amd import _lib
    res, args = _lib.SYMBOLS["nsc_map_rehash_dist"]
    assert res is C.c_int and C.c_size_t not in args and len(args) == 20
    assert "nsc_map_rehash_dist" not in W.wrapped_symbols() and len(W.wrapped_symbols()) == 28
    assert not [n for n, (r, _) in _lib.SYMBOLS.items() if "rehash" in n and r is C.c_size_t]
    assert [args[i] for i in (6, 7, 15)] == [C.c_int64, C.c_int32, C.c_int64]


def test_rehash_kernels_use_no_scratch(lib, tmp_path):
    """the four kernels of the move keep everything in registers (no scratch) and leave room for four waves per SIMD (at
    most 128 VGPRs); read from the gfx950 code object as test_map_replace_cpu.test_remove_and_replace_kernels_use_no_scratch
    does"""
    import kernel_budget as KB
    assert KB.binutils(), f"no llvm binutils in {KB.LLVM}"
    found = KB.kernels(r"rehash_(clear|count|scan|move)_kernel")
    assert len(found) == 4, sorted(found)
    for k, (vg, sc) in found.items():
        print(f"{k}: {vg} VGPRs, {sc} B scratch")
        assert sc == 0 and vg <= 128, f"{k}: {vg} VGPRs, {sc} B scratch"
