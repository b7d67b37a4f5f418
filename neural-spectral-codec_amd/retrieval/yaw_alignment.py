"""Yaw initial guess for stage 2 from the range images the encoder already builds (csrc/nsc_yaw.hip).

The descriptor is rotation invariant, so stage 1 retrieves a revisit whatever the heading difference; GICP is a
local method and from the identity converges for about 10 degrees of yaw.  A yaw between two scans of one place is
a circular shift of the 360 columns of the interpolated range image (``encode_points_batch(return_images=True)``,
third value), so the arg-max of the row-summed circular cross-correlation of the two images gives it to a degree
or so, which is well inside GICP's basin.

Definition (the contract nsc_yaw_align and tests/yaw_restatement.py share), all in float64, for two images
``Iq``, ``Ic`` of shape (R, 360), 1 <= R <= 64:

    a[r,c]   = Iq[r,c] - mean_c Iq[r,:]          b likewise from Ic
    score[s] = sum_r sum_c a[r,c] * b[r,(c - s) mod 360]                    s = 0 .. 359
    shift    = the s of the largest score, ties to the smaller s; 0 when that score is not > 0 (flat images)
    peak     = score[shift]
    runner_up = the largest score among shifts more than YAW_GUARD_BINS (10) bins from shift, circularly
    yaw      = -shift degrees, wrapped to (-180, 180]
    init     = Rz(yaw) as a (4,4) float64 matrix with zero translation: query into candidate coordinates;
               exactly the identity for shift 0

Images that are not finite.  One NaN or +-inf pixel among the R rows of either image makes its row mean, and with it
every one of the 360 scores, NaN.  Such a pair gets shift 0, the identity bit for bit, peak NaN and runner_up NaN,
so stage 2 starts it where it would start without a guess; ``yaw_info`` reports ``init_yaw_deg`` 0.0 and a NaN
``yaw_peak_ratio`` for it.  It stays distinct from a pair with an id outside its images, which gets shift -1 (and the
identity and NaN scores).  Finite float32 images, denormal or as large as 3.4e38, cannot overflow or underflow the
float64 sums: their scores are finite.

A candidate sensor yawed by +theta against the query gives ``shift ~ theta`` (mod 360).  The guess carries no
translation and no roll or pitch: a revisit offset by more than GICP's correspondence radius still needs odometry.
"""
from typing import List, Optional

import numpy as np
import torch

from .. import _lib
from .geometric_verification import _device, _ids

N_AZIMUTH = 360
MAX_ROWS = 64
YAW_GUARD_BINS = _lib.YAW_GUARD_BINS
# Largest batch handed to one nsc_yaw_align call (include/nsc.h NSC_YAW_MAX_PAIRS: threads per launch);
# estimate_yaw splits a larger request, with the same results bit for bit.  A module constant, so a test can lower it.
MAX_PAIRS_PER_CALL = _lib.YAW_MAX_PAIRS


def _images(x, device=None):
    """(R,360) or (B,R,360) host array or tensor -> (B,R,360) float32 tensor (on ``device`` if given)"""
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.asarray(x, dtype=np.float32))
    if t.ndim == 2:
        t = t[None]
    if t.ndim != 3 or int(t.shape[2]) != N_AZIMUTH or not 1 <= int(t.shape[1]) <= MAX_ROWS:
        raise _lib.NscError(f"range images must be (R,{N_AZIMUTH}) or (B,R,{N_AZIMUTH}) with 1 <= R <= {MAX_ROWS}, "
                            f"got {tuple(t.shape)}")
    t = t.detach().to(dtype=torch.float32)
    if device is not None:
        t = t.to(device)
    return t.contiguous()


class YawImages:
    """A device-resident store of interpolated range images, (R, 360) float32 each, for ``estimate_yaw``: an image's
    id is its insert order.  The buffer grows by amortised doubling; an image costs R * 1440 bytes (23 KB at 16
    rows).  R is that of the first image added (or ``rows=``)."""

    def __init__(self, rows: Optional[int] = None, device="cuda"):
        self.device = _device(device)
        self.rows = None if rows is None else int(rows)
        self._buf = None
        self._n = 0

    def __len__(self):
        return self._n

    @property
    def nbytes(self) -> int:
        """device bytes the store holds (its capacity)"""
        return 0 if self._buf is None else self._buf.numel() * self._buf.element_size()

    @property
    def images(self) -> torch.Tensor:
        """(len, R, 360) float32 device view of the images present"""
        if self._buf is None:
            return torch.empty((0, self.rows or 1, N_AZIMUTH), dtype=torch.float32, device=self.device)
        return self._buf[:self._n]

    def clear(self):
        """Forget every image; the buffer is kept for the next adds."""
        self._n = 0

    def add(self, images) -> List[int]:
        """Append one (R,360) image or a (B,R,360) batch (host array or device tensor) -> the new ids."""
        t = _images(images, self.device)
        B, R = int(t.shape[0]), int(t.shape[1])
        if self.rows is None:
            self.rows = R
        if R != self.rows:
            raise _lib.NscError(f"YawImages holds images of {self.rows} rows, got {R}")
        n = self._n
        cap = 0 if self._buf is None else int(self._buf.shape[0])
        if n + B > cap:
            nb = torch.empty((max(n + B, 2 * cap, 64), R, N_AZIMUTH), dtype=torch.float32, device=self.device)
            if n:
                nb[:n].copy_(self._buf[:n])
            self._buf = nb
        self._buf[n:n + B].copy_(t)
        self._n = n + B
        return list(range(n, n + B))


def estimate_yaw(query_images, query_ids, candidate_images, candidate_ids):
    """The yaw guess of pairs (query_ids[i], candidate_ids[i]) in one nsc_yaw_align launch.  ``*_images``: a
    YawImages store or an (n, R, 360) float32 device tensor (the two may be one); ids: device int64 tensors or host
    sequences.  Returns a dict of device tensors: shift (P,) int32, peak, runner_up (P,) float64 and
    init_transforms (P,4,4) float64 (query into candidate coordinates), as defined in the module docstring.
    Nothing is synchronised or allocated outside torch's allocator, so a call with device ids can be captured.  A
    pair with an id outside its images gets shift -1, NaN peak and runner_up and the identity; a pair with a NaN or
    +-inf pixel in either image gets shift 0, NaN peak and runner_up and the identity.  More than
    MAX_PAIRS_PER_CALL pairs go to the library in several calls, with the same results."""
    qi = query_images.images if isinstance(query_images, YawImages) else query_images
    ci = candidate_images.images if isinstance(candidate_images, YawImages) else candidate_images
    for t, name in ((qi, "query_images"), (ci, "candidate_images")):
        _lib.require_cuda(t, name)
        if t.dtype != torch.float32 or t.ndim != 3 or int(t.shape[2]) != N_AZIMUTH or not t.is_contiguous():
            raise _lib.NscError(f"{name} must be a contiguous (n, R, {N_AZIMUTH}) float32 tensor")
    dev = qi.device
    R = int(qi.shape[1])
    if ci.device != dev or int(ci.shape[1]) != R or not 1 <= R <= MAX_ROWS:
        raise _lib.NscError(f"estimate_yaw needs query and candidate images of the same 1..{MAX_ROWS} rows on one "
                            "device")
    qid, cid = _ids(query_ids, dev), _ids(candidate_ids, dev)
    P = int(qid.numel())
    if int(cid.numel()) != P:
        raise _lib.NscError("estimate_yaw needs as many candidate ids as query ids")
    if P > MAX_PAIRS_PER_CALL:
        step = MAX_PAIRS_PER_CALL
        parts = [estimate_yaw(qi, qid[a:a + step], ci, cid[a:a + step]) for a in range(0, P, step)]
        return {k: torch.cat([q[k] for q in parts], 0) for k in parts[0]}
    if qi.numel() == 0 or ci.numel() == 0:                   # no image: every id is invalid, nothing is read, but
        spare = torch.empty(1, dtype=torch.float32, device=dev)  # the library wants a pointer
        qi, ci = (qi if qi.numel() else spare), (ci if ci.numel() else spare)
    n_q, n_c = (int(t.shape[0]) if t.ndim == 3 else 0 for t in (qi, ci))
    shift = torch.empty(P, dtype=torch.int32, device=dev)
    scores = torch.empty((P, 2), dtype=torch.float64, device=dev)
    init = torch.empty((P, 4, 4), dtype=torch.float64, device=dev)
    _lib.call("nsc_yaw_align", dev, qi, n_q, ci, n_c, qid, cid, P, R, shift, scores, init, _lib.STREAM)
    return dict(shift=shift, peak=scores[:, 0], runner_up=scores[:, 1], init_transforms=init)


def yaw_info(shift: int, peak: float, runner_up: float) -> dict:
    """Host values of one pair -> the keys stage 2 adds to a candidate's info: ``init_yaw_deg`` (-shift wrapped to
    (-180, 180]; NaN for an invalid pair) and ``yaw_peak_ratio`` (peak / runner_up, inf when runner_up <= 0): a
    ratio near 1 marks an ambiguous pair.  A NaN peak (an image that is not finite, or an invalid id) gives a NaN
    ratio whatever runner_up is: such a pair says nothing about ambiguity."""
    shift = int(shift)
    peak, runner_up = float(peak), float(runner_up)
    deg = float("nan") if shift < 0 else float(-shift if shift < 180 else 360 - shift)
    if peak != peak:
        ratio = float("nan")
    else:
        ratio = peak / runner_up if runner_up > 0 else float("inf")
    return dict(init_yaw_deg=deg, yaw_peak_ratio=ratio)
