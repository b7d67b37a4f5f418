"""The move of a kept map to another capacity of include/nsc.h (nsc_map_rehash_dist) restated in numpy: the reference of
tests/test_map_rehash_cpu.py and tests/test_map_rehash_gpu.py.

The input is the kept tensors on the host (voxels, info, keys, stats and, when the map keeps them, moments and cursor, over
the full capacity).  The places below stats[1] are flagged kept or dropped, the kept ones are gathered in ascending order
with numpy's own indexing, and the index is a plain dict from key to place.  Nothing is computed: every number of the
destination is a number of the source."""
import numpy as np

TILE = 4096                              # include/nsc.h NSC_MAP_TILE_ROWS
NAMES = ("voxels_kept", "voxels_dropped", "source_keys_unplaced", "inconsistent_kept", "kept_unplaced", "kept_table_full")
FILL = dict(voxels=0.0, info=0, keys=0, moments=0)


def as_kept(m, cursor=None):
    """a map of the restatements (map_localize_restatement.build_dist's dict or map_insert_restatement.arrays) -> the kept
    tensors a build at its capacity leaves on the host; entries past stats[1] are zeros here"""
    cap, n = int(m["capacity"]), int(m["stats"][1])
    out = dict(voxels=np.zeros((cap, 16)), info=np.zeros((cap, 4), np.int64), keys=np.zeros(cap, np.int64),
               moments=np.zeros((cap, 9), np.int64), stats=np.array(m["stats"], np.int64))
    out["voxels"][:n], out["info"][:n], out["keys"][:n] = m["voxels"][:n], m["info"][:n], m["keys"][:n]
    out["moments"][:n] = np.array(m["moments"][:n].tolist(), np.int64).reshape(n, 9)
    cursor = m.get("cursor") if cursor is None else cursor
    if cursor is not None:
        out["cursor"] = np.array(cursor, np.int64)
    out["place"] = {int(k): (p if p < cap else -1) for k, p in m["place"].items()}
    return out


def kinds(k):
    """-> (emptied, inconsistent) flags of the places below stats[1]"""
    n = int(k["stats"][1])
    count = k["info"][:n, 0]
    clean = ~k["moments"][:n].any(1) if k.get("moments") is not None else np.ones(n, bool)
    emptied = (count == 0) & clean
    return emptied, (count < 0) | ((count == 0) & ~clean)


def rehash(k, keep_emptied, new_max_voxels):
    """kept tensors on the host -> the destination tensors (entries past the new stats[1] are zeros here), new_place,
    tile_base, rehashed, and ``place`` {key: place or -1}, None when more voxels are kept than the new index has slots"""
    M, N = len(k["info"]), int(new_max_voxels)
    found, written = int(k["stats"][0]), int(k["stats"][1])
    emptied, inconsistent = kinds(k)
    keep = np.ones(written, bool) if keep_emptied else ~emptied
    old = np.nonzero(keep)[0]
    kept, n = len(old), min(len(old), N)
    new_place = np.full(M, -1, np.int64)
    new_place[old[:n]] = np.arange(n)
    tiles = -(-M // TILE)
    flags = np.zeros(tiles * TILE, np.int64)
    flags[old] = 1
    tile_base = np.concatenate([[0], np.cumsum(flags.reshape(tiles, TILE).sum(1))]).astype(np.int64)
    out = dict(new_place=new_place, tile_base=tile_base,
               stats=np.array([kept, n] + k["stats"][2:].tolist(), np.int64),
               rehashed=np.array([kept, written - kept, found - written, int(inconsistent[keep].sum()), kept - n,
                                  max(0, kept - 2 * N)], np.int64))
    for name in ("voxels", "info", "keys", "moments"):
        if k.get(name) is not None:
            out[name] = np.full((N,) + k[name].shape[1:], FILL[name], k[name].dtype)
            out[name][:n] = k[name][old[:n]]
    if k.get("cursor") is not None:
        out["cursor"] = k["cursor"].copy()
    out["place"] = None if kept > 2 * N else {int(key): (q if q < N else -1) for q, key in enumerate(k["keys"][old].tolist())}
    return out
