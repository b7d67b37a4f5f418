"""The yaw initial guess on the MI355X: nsc_yaw_align (estimate_yaw) against the float64 restatement
(tests/yaw_restatement.py) on encoder images, random images and planted shifts; flat images, invalid ids, batch limits,
determinism, hipGraph capture together with the registration; the constructed cases of tests/yaw_cases.py (exact ties,
chunk edges, denormal and very large pixels: bit for bit against an int64 reference; images that are not finite); and
the loop-closing paths that use the guess."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import gicp_restatement as G
import yaw_cases as C
import yaw_restatement as Y
from neural_spectral_codec_amd import synth
from test_gicp_cpu import R_BAR, REVISITS, T_BAR, revisit
from test_yaw_cpu import MARGIN, ROTATED, UNGUESSED, YAW_BAR_DEG

pytestmark = pytest.mark.gpu

PEAK_RTOL = 1e-9         # float64 sums of at most 92 160 terms are good to about 1e-11 of the peak
INIT_ATOL = 1e-15        # a few ulp of a value <= 1
IDENTITY = np.eye(4).tobytes()


def _ya():
    from neural_spectral_codec_amd.retrieval import yaw_alignment as ya
    return ya


def estimate(qi, qids, ci, cids):
    out = _ya().estimate_yaw(qi, qids, ci, cids)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()


def assert_matches(got, i, Iq, Ic, what=""):
    """pair i of estimate_yaw's outputs against the restatement of its two images (which must not be a tie)"""
    r = Y.align(Iq, Ic)
    print(what, "shift", got["shift"][i], r["shift"], "peak", got["peak"][i], r["peak"], "runner_up",
          got["runner_up"][i], r["runner_up"])
    assert r["peak"] > 0 and r["peak"] - r["second"] > MARGIN * r["peak"], (what, r["peak"], r["second"])
    assert got["shift"][i] == r["shift"], (what, got["shift"][i], r["shift"])
    assert abs(got["peak"][i] - r["peak"]) <= PEAK_RTOL * abs(r["peak"]), what
    assert abs(got["runner_up"][i] - r["runner_up"]) <= PEAK_RTOL * abs(r["peak"]), what
    if r["shift"] == 0:
        assert got["init_transforms"][i].tobytes() == IDENTITY, what
    else:
        assert np.max(np.abs(got["init_transforms"][i] - r["init"])) <= INIT_ATOL, what
    return r


def assert_same(a, i, b, j, what=""):
    for k in ("shift", "peak", "runner_up", "init_transforms"):
        x, y = np.ascontiguousarray(a[k][i]), np.ascontiguousarray(b[k][j])
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), (what, i, j, k, x, y)


@pytest.fixture(scope="module")
def encoder():
    from neural_spectral_codec_amd.encoding import SpectralEncoder
    return SpectralEncoder(n_elevation=16).to("cuda")


@pytest.fixture(scope="module")
def rotated():
    return [revisit(o, None) for o in ROTATED]


@pytest.fixture(scope="module")
def revisits():
    return [revisit(o, g) for o, g in REVISITS]


@pytest.fixture(scope="module")
def other():
    return synth.scan_world(synth.make_world(11, ground_z=-4.0), synth.pose_xyz_yaw(0, 0), seed=5)


def test_encoder_images_match_restatement(encoder, rotated, revisits):
    cases = [(o, p) for o, p in zip(ROTATED, rotated)] + [(o, p) for (o, _), p in zip(REVISITS, revisits)]
    A = cases[0][1][0]
    clouds = [A] + [p[1] for _, p in cases]
    images = encoder.encode_points_batch(clouds, return_images=True)[2]
    assert tuple(images.shape) == (len(clouds), 16, 360)
    P = len(cases)
    got = estimate(images, [0] * P, images, list(range(1, P + 1)))
    host = images.cpu().numpy()
    for i, (o, _) in enumerate(cases):
        r = assert_matches(got, i, host[0], host[i + 1], o)
        assert abs(Y.wrap_deg(r["yaw_deg"] + o[2])) <= YAW_BAR_DEG, (o, r["shift"])


@pytest.mark.parametrize("R", [1, 7, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64])
def test_random_images_match_restatement(R):
    rng = np.random.default_rng(100 + R)
    q = rng.uniform(0.0, 80.0, (3, R, 360)).astype(np.float32)
    c = rng.uniform(0.0, 80.0, (4, R, 360)).astype(np.float32)
    c[1] = np.roll(q[2], -201, axis=1) + rng.normal(0, 1.0, (R, 360)).astype(np.float32)     # a noisy rotated copy
    c[3, :, ::3] = 0.0                                                                       # empty columns
    pl = [(0, 0), (2, 1), (1, 3), (2, 2), (0, 3), (1, 1)]
    got = estimate(dev(q), [a for a, _ in pl], dev(c), [b for _, b in pl])
    for i, (a, b) in enumerate(pl):
        r = assert_matches(got, i, q[a], c[b], (R, a, b))
        if (a, b) == (2, 1):
            assert r["shift"] == 201
    same = estimate(dev(q), [0, 1], dev(q), [1, 0])          # both sides one array
    assert_matches(same, 0, q[0], q[1], (R, "same array"))
    assert_matches(same, 1, q[1], q[0], (R, "same array"))


def test_planted_shifts():
    rng = np.random.default_rng(5)
    base = rng.uniform(1.0, 80.0, (16, 360)).astype(np.float32)
    c = np.stack([np.roll(base, -s, axis=1) for s in range(360)])        # the candidate sensor yawed by +s bins
    got = estimate(dev(base[None]), [0] * 360, dev(c), list(range(360)))
    assert np.array_equal(got["shift"], np.arange(360, dtype=np.int32))
    for s in range(360):
        assert_matches(got, s, base, c[s], s)
    yaw = np.rad2deg(np.arctan2(got["init_transforms"][:, 1, 0], got["init_transforms"][:, 0, 0]))
    assert np.all(np.abs(Y.wrap_deg(yaw + np.arange(360))) < 1e-9)       # Rz(-shift), wrapped to (-180, 180]
    assert yaw.min() > -180.0 and np.isclose(yaw.max(), 180.0)
    rest = got["init_transforms"].copy()
    rest[:, :2, :2] = 0
    assert np.all(rest == np.eye(4) - np.diag([1.0, 1, 0, 0]))           # no translation, nothing else


def test_flat_and_zero_images():
    rng = np.random.default_rng(6)
    some = rng.uniform(1.0, 80.0, (16, 360)).astype(np.float32)
    flat = np.repeat(rng.uniform(1.0, 80.0, (16, 1)).astype(np.float32), 360, axis=1)   # every row constant
    imgs = np.stack([some, flat, np.zeros((16, 360), np.float32)])
    pl = [(1, 0), (0, 1), (1, 1), (2, 0), (0, 2), (2, 2), (1, 2)]
    got = estimate(dev(imgs), [a for a, _ in pl], dev(imgs), [b for _, b in pl])
    for i in range(len(pl)):
        assert got["shift"][i] == 0 and got["peak"][i] == 0.0 and got["runner_up"][i] == 0.0, pl[i]
        assert got["init_transforms"][i].tobytes() == IDENTITY


def test_invalid_ids():
    rng = np.random.default_rng(7)
    q = rng.uniform(0.0, 80.0, (2, 16, 360)).astype(np.float32)
    c = rng.uniform(0.0, 80.0, (3, 16, 360)).astype(np.float32)
    qids = torch.tensor([0, -1, 1, 2, 0, 1, 1 << 40, 1], dtype=torch.int64, device="cuda")
    cids = torch.tensor([2, 0, 1, 0, 3, -5, 0, 0], dtype=torch.int64, device="cuda")
    got = estimate(dev(q), qids, dev(c), cids)
    ref = estimate(dev(q), [0, 1, 1], dev(c), [2, 1, 0])
    for i, j in ((0, 0), (2, 1), (7, 2)):                    # the valid pairs beside them are unchanged
        assert_same(got, i, ref, j, "beside")
    assert_matches(got, 0, q[0], c[2])
    for i in (1, 3, 4, 5, 6):
        assert got["shift"][i] == -1 and np.isnan(got["peak"][i]) and np.isnan(got["runner_up"][i]), i
        assert got["init_transforms"][i].tobytes() == IDENTITY, i
    store = _ya().YawImages(rows=16)                         # an empty store: every id is invalid
    got = estimate(store, [0], dev(c), [0])
    assert got["shift"][0] == -1 and got["init_transforms"][0].tobytes() == IDENTITY


# ------------------------------------------------------------------------------------------------
# the constructed cases of yaw_cases.py
# ------------------------------------------------------------------------------------------------
def assert_bits(got, i, want, what=""):
    """pair i of estimate_yaw's outputs against yaw_cases.expected, bit for bit"""
    for k in ("shift", "peak", "runner_up", "init_transforms"):
        x, y = np.ascontiguousarray(got[k][i]), np.ascontiguousarray(want[k])
        assert x.dtype == y.dtype and x.shape == y.shape, (what, k, x.dtype, y.dtype)
        assert x.tobytes() == y.tobytes(), (what, k, x, y)


def assert_not_finite_contract(got, i, what=""):
    """a pair with a pixel that is not finite: shift 0 (not -1), the identity bit for bit, peak NaN, runner_up NaN"""
    print(what, "shift", got["shift"][i], "peak", got["peak"][i], "runner_up", got["runner_up"][i])
    assert got["shift"][i] == 0, (what, got["shift"][i])
    assert got["init_transforms"][i].tobytes() == IDENTITY, what
    assert np.isnan(got["peak"][i]), (what, got["peak"][i])
    assert np.isnan(got["runner_up"][i]), (what, got["runner_up"][i])


def test_exact_cases_bit_for_bit():
    """Integer images whose float64 scores are exact in any order: two-way ties wherever the arg-max decides them (one
    scan lane, across the butterfly, across the waves and lanes of the sums), the informative row at every chunk and
    group edge, three-, four- and 72-way ties, and the same with denormal and with 2^100-scaled pixels.  One launch
    per row count; every output equals the int64 reference's, with no tolerance."""
    groups = C.by_rows(C.exact_cases())
    assert sorted(groups) == [1, 15, 16, 17, 31, 33, 48, 49, 63, 64]
    for R, cases in sorted(groups.items()):
        n = len(cases)
        got = estimate(dev(np.stack([c.Iq for c in cases])), list(range(n)),
                       dev(np.stack([c.Ic for c in cases])), list(range(n)))
        for i, c in enumerate(cases):
            e = C.expected(c)
            print(c.name, "shift", got["shift"][i], e["shift"], "peak", got["peak"][i], e["peak"], "runner_up",
                  got["runner_up"][i], e["runner_up"])
            assert (int(e["shift"]), float(e["peak"]), float(e["runner_up"])) == (c.shift, c.peak, c.runner_up), c.name
            assert_bits(got, i, e, c.name)


def test_tie_alone_and_between_ordinary_pairs():
    rng = np.random.default_rng(12)
    some = rng.uniform(0.0, 80.0, (4, 17, 360)).astype(np.float32)
    ties = [C.delta(17, 16, 63, 64), C.delta(17, 16, 0, 64), C.delta(17, 16, 100, 300)]
    q = np.concatenate([some[:2], np.stack([c.Iq for c in ties])])
    c = np.concatenate([some[2:], np.stack([c.Ic for c in ties])])
    pl = [(0, 0), (2, 2), (1, 1), (3, 3), (0, 1), (4, 4), (1, 0)]
    got = estimate(dev(q), [a for a, _ in pl], dev(c), [b for _, b in pl])
    for i, (a, b) in enumerate(pl):
        if a >= 2:
            assert a == b
            assert_bits(got, i, C.expected(ties[a - 2]), ties[a - 2].name)
            alone = estimate(dev(ties[a - 2].Iq[None]), [0], dev(ties[a - 2].Ic[None]), [0])
            assert_same(alone, 0, got, i, "alone")
        else:
            assert_matches(got, i, q[a], c[b], (a, b))


def test_finite_maximum():
    Iq, Ic, planted = C.finite_maximum()
    got = estimate(dev(Iq[None]), [0], dev(Ic[None]), [0])
    r = assert_matches(got, 0, Iq, Ic, "3.4e38")
    assert r["shift"] == planted == 2 and np.isfinite(got["peak"][0]) and np.isfinite(got["runner_up"][0])


@pytest.mark.parametrize("R", [1, 16, 17])
def test_images_that_are_not_finite(R):
    """NaN, +inf, -inf and +inf with -inf in one row; in the query, the candidate and both; in the first row and in the
    last (for 17 rows the last is alone in its chunk).  Every such pair gets (0, identity, NaN, NaN), and the valid pairs
    of the same launch keep the bits of a launch without them."""
    rng = np.random.default_rng(40 + R)
    good_q = rng.uniform(0.0, 80.0, (2, R, 360)).astype(np.float32)
    good_c = rng.uniform(0.0, 80.0, (2, R, 360)).astype(np.float32)
    bad = C.nonfinite_pairs(R)
    q = np.concatenate([good_q, np.stack([p[1] for p in bad])])
    c = np.concatenate([good_c, np.stack([p[2] for p in bad])])
    valid = [(0, 0), (1, 1), (0, 1)]
    at = {0: valid[0], len(bad) // 2 + 1: valid[1], len(bad) + 2: valid[2]}      # first, in the middle, last
    pl, k = [], 0
    for i in range(len(bad) + 3):
        if i in at:
            pl.append(at[i])
        else:
            pl.append((2 + k, 2 + k))
            k += 1
    assert k == len(bad) and pl[0] == valid[0] and pl[-1] == valid[2]
    got = estimate(dev(q), [a for a, _ in pl], dev(c), [b for _, b in pl])
    ref = estimate(dev(good_q), [a for a, _ in valid], dev(good_c), [b for _, b in valid])
    for i, (a, b) in enumerate(pl):
        if i in at:
            j = valid.index((a, b))
            assert_same(got, i, ref, j, "beside")
            assert_matches(got, i, good_q[a], good_c[b], ("beside", a, b))
        else:
            assert_not_finite_contract(got, i, bad[a - 2][0])
    # a clean image against a poisoned one of the other array, and an invalid id beside them: -1 stays -1
    mixed = estimate(dev(q), [0, 2, 0, 5], dev(c), [2, 0, len(c), 5])
    assert not np.isfinite(q[2]).all() and np.isfinite(c[2]).all() and np.isfinite(q[0]).all()
    assert_matches(mixed, 0, q[0], c[2], "clean query, clean candidate of a poisoned pair")
    assert_not_finite_contract(mixed, 1, "poisoned query, clean candidate")
    assert mixed["shift"][2] == -1 and np.isnan(mixed["peak"][2]) and np.isnan(mixed["runner_up"][2])
    assert mixed["init_transforms"][2].tobytes() == IDENTITY
    assert_not_finite_contract(mixed, 3, bad[3][0])


def test_empty_and_split_batches(monkeypatch):
    ya = _ya()
    rng = np.random.default_rng(8)
    q = dev(rng.uniform(0.0, 80.0, (5, 16, 360)))
    c = dev(rng.uniform(0.0, 80.0, (6, 16, 360)))
    none = estimate(q, [], c, [])
    assert none["shift"].shape == (0,) and none["peak"].shape == (0,) and none["init_transforms"].shape == (0, 4, 4)
    qids = [i % 5 for i in range(23)]
    cids = [(7 * i) % 6 for i in range(23)]
    cids[11] = 6                                              # an invalid pair inside a chunk
    whole = estimate(q, qids, c, cids)
    monkeypatch.setattr(ya, "MAX_PAIRS_PER_CALL", 5)
    split = estimate(q, qids, c, cids)
    parts = [estimate(q, qids[a:a + 5], c, cids[a:a + 5]) for a in range(0, 23, 5)]
    assert split["shift"].shape == (23,) and split["init_transforms"].shape == (23, 4, 4)
    at = 0
    for part in parts:
        for j in range(len(part["shift"])):
            assert_same(split, at, part, j, "chunk")
            assert_same(split, at, whole, at, "whole")
            at += 1
    assert at == 23 and whole["shift"][11] == -1


def test_deterministic_and_batch_independent():
    rng = np.random.default_rng(9)
    q = rng.uniform(0.0, 80.0, (4, 64, 360)).astype(np.float32)
    c = rng.uniform(0.0, 80.0, (4, 64, 360)).astype(np.float32)
    pl = [(a, b) for a in range(4) for b in range(4)]
    one = estimate(dev(q), [a for a, _ in pl], dev(c), [b for _, b in pl])
    two = estimate(dev(q), [a for a, _ in pl], dev(c), [b for _, b in pl])
    for i in range(len(pl)):
        assert_same(one, i, two, i, "second run")
    perm = rng.permutation(len(pl))
    shuffled = estimate(dev(q), [pl[k][0] for k in perm], dev(c), [pl[k][1] for k in perm])
    for i, k in enumerate(perm):
        assert_same(shuffled, i, one, k, "order")
    single = estimate(dev(q[2:3]), [0], dev(c[1:2]), [0])    # alone, in arrays of its own
    assert_same(single, 0, one, pl.index((2, 1)), "single")
    many = estimate(dev(q), [2] * 700, dev(c), [1] * 700)    # more pairs than CUs
    for i in (0, 255, 256, 699):
        assert_same(many, i, one, pl.index((2, 1)), "large batch")


def test_yaw_image_store():
    ya = _ya()
    rng = np.random.default_rng(10)
    imgs = rng.uniform(0.0, 80.0, (150, 16, 360)).astype(np.float32)
    store = ya.YawImages()
    assert len(store) == 0 and store.nbytes == 0
    assert store.add(imgs[0]) == [0]                         # one (R,360) host image
    assert store.add(dev(imgs[1:3])) == [1, 2]               # a device batch
    sizes = [store.nbytes]
    for i in range(3, 150):
        assert store.add(imgs[i]) == [i]
        sizes.append(store.nbytes)
    assert len(store) == 150 and len(set(sizes)) == 3        # 64 -> 128 -> 256 images: amortised doubling
    assert store.nbytes == 256 * 16 * 360 * 4
    assert store.images.cpu().numpy().tobytes() == imgs.tobytes()
    with pytest.raises(ya._lib.NscError):
        store.add(np.zeros((8, 360), np.float32))            # another row count
    with pytest.raises(ya._lib.NscError):
        store.add(np.zeros((16, 180), np.float32))
    got = estimate(store, [0, 149, 70], store, [149, 3, 70])
    ref = estimate(dev(imgs), [0, 149, 70], dev(imgs), [149, 3, 70])
    for i in range(3):
        assert_same(got, i, ref, i, "store")
    nbytes = store.nbytes
    store.clear()
    assert len(store) == 0 and store.add(imgs[5:7]) == [0, 1] and store.nbytes == nbytes
    got = estimate(store, [0, 2], store, [1, 0])
    assert_matches(got, 0, imgs[5], imgs[6])
    assert got["shift"][1] == -1                             # ids count the images present, not the capacity


def test_capture_with_registration(encoder, rotated):
    from _hipgraph import keep_graphs, node_types
    from neural_spectral_codec_amd.retrieval import geometric_verification as gv
    A = rotated[0][0]
    clouds = [A, rotated[0][1], rotated[1][1], rotated[3][1]]
    store = gv.PreparedClouds()
    store.add(clouds)
    images = _ya().YawImages()
    images.add(encoder.encode_points_batch(clouds, return_images=True)[2])
    sids = torch.tensor([0, 0, 0], dtype=torch.int64, device="cuda")
    tids = torch.tensor([1, 2, 3], dtype=torch.int64, device="cuda")

    def step():
        yaw = _ya().estimate_yaw(images, sids, images, tids)
        out = gv.register_prepared(store, sids, store, tids, yaw["init_transforms"])
        return {**yaw, **out}
    eager = {k: v.clone() for k, v in step().items()}
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()                                               # warm the allocator outside the capture
    torch.cuda.current_stream().wait_stream(s)
    with keep_graphs() as made:
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            cap = step()
    g.replay()
    torch.cuda.synchronize()
    for k in eager:
        assert torch.equal(eager[k], cap[k]), k
    types = node_types(made[0])
    assert types.get("memset", 0) == 0 and types.get("memcpy", 0) == 0, types
    assert types.get("kernel", 0) == (1 + 2 * 31) + 1        # the registration's launches and the yaw launch
    for i, k in enumerate((0, 1, 3)):                        # and the captured pairs converged
        te, re = G.pose_error(cap["transform"][i].cpu().numpy(), rotated[k][2])
        assert te <= T_BAR and re <= R_BAR, (k, te, np.rad2deg(re))


# ------------------------------------------------------------------------------------------------
# loop closing
# ------------------------------------------------------------------------------------------------
def _edge_fn(source_pose, target_pose, relative_transform, information_matrix):
    return {"transform": relative_transform, "information": information_matrix}


def _database(targets, other, n_queries=1):
    rng = np.random.default_rng(0)
    n = len(targets) + 1
    desc = rng.random((n + n_queries, 800)).astype(np.float32)
    desc /= desc.sum(1, keepdims=True)
    kfs = [SimpleNamespace(keyframe_id=100 + i, scan_id=i, points=s, descriptor=desc[i], pose=None)
           for i, s in enumerate(list(targets) + [other])]
    return kfs, desc[n:]


def _retrieval(kfs, **kw):
    from neural_spectral_codec_amd.retrieval import GeometricVerifier, create_two_stage_retrieval
    r = create_two_stage_retrieval(top_k=len(kfs), verifier=GeometricVerifier(), edge_fn=_edge_fn, **kw)
    r.add_keyframes(kfs[:3])
    for kf in kfs[3:]:
        r.add_keyframe(kf)
    return r


def _same_closures(a, b):
    assert [e["target_id"] for e in a] == [e["target_id"] for e in b]
    for x, y in zip(a, b):
        assert x.keys() == y.keys()
        for k in x:
            assert np.asarray(x[k]).tobytes() == np.asarray(y[k]).tobytes(), k


def test_rotated_revisits_close_the_loop(rotated, other):
    """The database holds the six rotated revisits of the query's place and a scan of another world.  With the yaw
    guess exactly the six come back, each with the true relative pose; from the identity GICP settles on the ground
    plane and loop edges come back with a rotation that is wrong by more than 45 degrees."""
    kfs, qdesc = _database([p[1] for p in rotated], other)
    query = SimpleNamespace(keyframe_id=7, scan_id=7, points=rotated[0][0], descriptor=qdesc[0], pose=None)
    truth = {100 + i: p[2] for i, p in enumerate(rotated)}

    with_yaw = _retrieval(kfs, yaw_init=True)
    assert len(with_yaw.yaw_images) == 7 and with_yaw.yaw_images.rows == 16
    edges = with_yaw.get_loop_closures(query)
    assert sorted(e["target_id"] for e in edges) == sorted(truth)
    for e in edges:
        te, re = G.pose_error(e["transform"], truth[e["target_id"]])
        print("yaw_init", e["target_id"], "translation error", te, "rotation error deg", np.rad2deg(re), e["fitness"])
        assert te <= T_BAR and re <= R_BAR, (e["target_id"], te, np.rad2deg(re))

    # info: the two new keys; the guess is within the bar of the true yaw; the other world is looked at and rejected
    everyone = with_yaw._global_retrieval(query)
    verified = with_yaw._geometric_verification(query.points, everyone, query_image=with_yaw._range_images([query]))
    assert len(everyone) == 7 and len(verified) == 6
    for c in everyone:
        assert {"init_yaw_deg", "yaw_peak_ratio", "fitness", "rmse"} <= set(c.info)
        if c.database_idx < 6:
            assert c.verified and c.info["yaw_peak_ratio"] > 1.0
            assert abs(Y.wrap_deg(c.info["init_yaw_deg"] + ROTATED[c.database_idx][2])) <= YAW_BAR_DEG
        else:
            assert not c.verified

    # both stage-2 modes: bitwise the same
    prepared = _retrieval(kfs, yaw_init=True, prepare_geometry=True)
    _same_closures(edges, prepared.get_loop_closures(query))
    prepared.clear_database()
    assert len(prepared.yaw_images) == 0 and len(prepared.geometry) == 0 and prepared.query(query) == []

    # today's path: verified, and wrong
    without = _retrieval(kfs, yaw_init=False)
    assert without.yaw_images is None and without.yaw_encoder is None
    wrong = 0
    for e in without.get_loop_closures(query):
        if e["target_id"] in truth:
            _, re = G.pose_error(e["transform"], truth[e["target_id"]])
            print("identity", e["target_id"], "rotation error deg", np.rad2deg(re), e["fitness"], e["rmse"])
            wrong += np.rad2deg(re) > 45.0
    assert wrong >= 1


def test_batch_loop_closing_with_yaw(rotated, other, monkeypatch):
    from neural_spectral_codec_amd.retrieval import GeometricVerifier, batch_loop_closing
    ya = _ya()
    kfs, qdesc = _database([p[1] for p in rotated[:3]], other, n_queries=2)
    queries = [SimpleNamespace(keyframe_id=7, points=rotated[0][0], descriptor=qdesc[0], pose=None),
               SimpleNamespace(keyframe_id=8, points=rotated[5][1], descriptor=qdesc[1], pose=None)]
    per_query = batch_loop_closing(queries, kfs, top_k=4, verifier=GeometricVerifier(), edge_fn=_edge_fn,
                                   yaw_init=True)
    calls = []
    orig = ya.estimate_yaw

    def counted(*a, **kw):
        calls.append(len(a[1]))
        return orig(*a, **kw)
    monkeypatch.setattr(ya, "estimate_yaw", counted)
    batched = batch_loop_closing(queries, kfs, top_k=4, verifier=GeometricVerifier(), edge_fn=_edge_fn,
                                 prepare_geometry=True, yaw_init=True)
    assert calls == [2 * 4]                                  # every query's pairs in one estimate
    assert set(batched) == set(per_query) == {0, 1}
    for i in per_query:
        _same_closures(per_query[i], batched[i])
    assert {e["target_id"] for e in batched[0]} == {100, 101, 102}
    # the second query is itself a rotated scan of the place: 137.3 degrees against 90, 180 and -120, within 0.8 m
    # (the other world is not asserted for it: from some starts GICP pulls two ground planes together and the default
    # thresholds pass on the ground alone)
    assert {e["target_id"] for e in batched[1]} >= {100, 101, 102}
    for e in (e for e in batched[1] if e["target_id"] != 103):
        T_true = rotated[e["target_id"] - 100][2] @ np.linalg.inv(rotated[5][2])
        te, re = G.pose_error(e["transform"], T_true)
        assert te <= T_BAR and re <= R_BAR, (e["target_id"], te, np.rad2deg(re))


def test_small_revisits_still_verify(other):
    pairs = [revisit(o, None) for o in UNGUESSED]
    kfs, qdesc = _database([p[1] for p in pairs], other)
    query = SimpleNamespace(keyframe_id=7, points=pairs[0][0], descriptor=qdesc[0], pose=None)
    for prep in (False, True):
        edges = _retrieval(kfs, yaw_init=True, prepare_geometry=prep).get_loop_closures(query)
        assert sorted(e["target_id"] for e in edges) == [100, 101, 102]
        for e in edges:
            te, re = G.pose_error(e["transform"], pairs[e["target_id"] - 100][2])
            assert te <= T_BAR and re <= R_BAR, (e["target_id"], te, np.rad2deg(re))


def test_keyframe_range_image_is_used(encoder, rotated, other):
    """A keyframe that carries its interpolated range image is not encoded again; the results are the same."""
    kfs, qdesc = _database([p[1] for p in rotated[:2]], other)
    query = SimpleNamespace(keyframe_id=7, points=rotated[0][0], descriptor=qdesc[0], pose=None)
    ref = _retrieval(kfs, yaw_init=True).get_loop_closures(query)
    images = encoder.encode_points_batch([kf.points for kf in kfs] + [query.points], return_images=True)[2]
    for kf, im in zip(kfs + [query], images):
        kf.range_image = im.cpu().numpy()

    class NoEncoder:
        def encode_points_batch(self, *a, **kw):
            raise AssertionError("the keyframes carry their images")
    _same_closures(ref, _retrieval(kfs, yaw_init=True, yaw_encoder=NoEncoder()).get_loop_closures(query))


def test_keyframe_image_with_a_nan_pixel(encoder, rotated, other):
    """A database keyframe whose range_image holds one NaN pixel: its pair starts from the identity, as it would without
    the guess, and says so (init_yaw_deg 0.0, yaw_peak_ratio NaN, not inf); the other candidates do not notice."""
    targets = [p[1] for p in rotated[:3]]
    poisoned_idx = 1
    clouds = targets + [other, rotated[0][0]]
    images = encoder.encode_points_batch(clouds, return_images=True)[2].cpu().numpy()
    assert np.isfinite(images).all()

    def candidates(poison, **kw):
        kfs, qdesc = _database(targets, other)
        query = SimpleNamespace(keyframe_id=7, scan_id=7, points=rotated[0][0], descriptor=qdesc[0], pose=None)
        for kf, im in zip(kfs + [query], images):
            kf.range_image = im.copy()
        if poison:
            kfs[poisoned_idx].range_image[9, 200] = np.nan
        r = _retrieval(kfs, **kw)
        everyone = r._global_retrieval(query)                # verified or not
        r._geometric_verification(query.points, everyone,
                                  query_image=r._range_images([query]) if r.yaw_images is not None else None)
        assert len(everyone) == 4
        return {c.database_idx: c for c in everyone}

    def same_result(x, y):
        assert x.verified == y.verified and x.fitness == y.fitness and x.rmse == y.rmse
        assert np.asarray(x.transform).tobytes() == np.asarray(y.transform).tobytes()

    bad = candidates(True, yaw_init=True)
    clean = candidates(False, yaw_init=True)
    identity = candidates(False, yaw_init=False)
    c = bad[poisoned_idx]
    assert c.info["init_yaw_deg"] == 0.0 and np.isnan(c.info["yaw_peak_ratio"]), c.info
    assert not np.isnan(c.fitness) and np.isfinite(np.asarray(c.transform)).all()
    same_result(c, identity[poisoned_idx])                   # it started from the identity
    assert clean[poisoned_idx].info["init_yaw_deg"] != 0.0 and clean[poisoned_idx].info["yaw_peak_ratio"] > 1.0
    for i in (0, 2, 3):                                      # the others: bitwise what they are without the poison
        same_result(bad[i], clean[i])
        assert bad[i].info["init_yaw_deg"] == clean[i].info["init_yaw_deg"]
        assert bad[i].info["yaw_peak_ratio"] == clean[i].info["yaw_peak_ratio"]


def test_off_is_todays_path(revisits, other, monkeypatch):
    from neural_spectral_codec_amd import _lib
    from neural_spectral_codec_amd.retrieval import GeometricVerifier, TwoStageRetrieval
    kfs, qdesc = _database([revisits[0][1], revisits[1][1]], other)
    query = SimpleNamespace(keyframe_id=7, points=revisits[0][0], descriptor=qdesc[0], pose=None)
    called = []
    monkeypatch.setattr(_ya(), "estimate_yaw", lambda *a, **kw: called.append(1))
    for prep in (False, True):
        plain = _retrieval(kfs, prepare_geometry=prep)
        off = _retrieval(kfs, prepare_geometry=prep, yaw_init=False)
        a, b = plain.query(query), off.query(query)
        assert [c.database_idx for c in a] == [c.database_idx for c in b] and len(a) == 2
        for x, y in zip(a, b):
            assert x.verified == y.verified and x.distance == y.distance
            assert x.fitness == y.fitness and x.rmse == y.rmse
            assert x.transform.tobytes() == y.transform.tobytes()
            assert x.information_matrix.tobytes() == y.information_matrix.tobytes()
            assert "init_yaw_deg" not in x.info and "init_yaw_deg" not in y.info
    assert not called

    class OldVerifier:                                       # stage 2 without initial transforms
        def verify(self, query_points, candidate_points):
            return False, np.eye(4), dict(fitness=0.0, rmse=0.0)

        def verify_batch(self, query_points, candidate_points_list):
            return [self.verify(query_points, c) for c in candidate_points_list]
    TwoStageRetrieval(verifier=OldVerifier())
    for kw in (dict(verifier=OldVerifier()), dict(verifier=None), dict(verifier=GeometricVerifier(), prepare_geometry=True,
                                                                       yaw_encoder=None)):
        if isinstance(kw.get("verifier"), GeometricVerifier):
            TwoStageRetrieval(yaw_init=True, **kw)           # supported: constructs
            continue
        with pytest.raises(_lib.NscError):
            TwoStageRetrieval(yaw_init=True, **kw)
