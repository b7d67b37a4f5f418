"""Constructed inputs of tests/test_map_replace_cpu.py and tests/test_map_replace_gpu.py, beside those of
tests/map_insert_cases.py and tests/map_localize_cases.py.  The CPU file asserts what each case claims about itself; the
GPU file relies on it."""
import numpy as np

import map_insert_cases as IK
import map_localize_cases as K
import map_restatement as M

B_SHIFT = np.array([0.37, -0.21, 0.05])      # metres by which general_split's group B is re-placed
SCENE_MOVED = (2, 3)                         # the scene's clouds that a closure moves
SCENE_SHIFT, SCENE_TURN = np.array([0.48, -0.36, 0.0]), np.deg2rad(2.0)      # 0.6 m and 2 degrees
# update_prepared: cloud 1 moves by less than both thresholds, the clouds of SCENE_MOVED by more than both
MIN_TRANSLATION, MIN_ROTATION = 0.05, np.deg2rad(0.5)
SMALL_SHIFT = np.array([1e-3, 0.0, 0.0])


def shifted(poses, d):
    """the poses with ``d`` added to every translation (a shift in the world)"""
    out = np.array(poses, np.float64)
    out[:, :3, 3] += np.asarray(d, np.float64)
    return out


def one_voxel_on(poses):
    """B's poses of IK.sized_insert moved by one voxel along x: lattice coordinates stay exact"""
    return shifted(poses, [1.0, 0.0, 0.0])


def scene_new_poses():
    """K.scene's six poses with the clouds of SCENE_MOVED turned by SCENE_TURN about z and shifted by SCENE_SHIFT, and
    the same with cloud 1 moved by SMALL_SHIFT besides -> (new poses, new poses with the small move)"""
    poses = K.scene()["poses"]
    new = poses.copy()
    turn = K.general_pose(SCENE_TURN, 0.0, [0.0, 0.0, 0.0])[:3, :3]
    for c in SCENE_MOVED:                        # turned about the sensor's own position, then shifted
        new[c, :3, :3] = turn @ poses[c, :3, :3]
        new[c, :3, 3] = poses[c, :3, 3] + SCENE_SHIFT
    small = new.copy()
    small[1] = shifted(poses[1:2], SMALL_SHIFT)[0]
    return new, small


def scene_cloud_group(ids):
    """the scene's clouds ``ids`` -> (points, offsets)"""
    s = K.scene()
    return IK.pack([s["points"][4000 * c:4000 * (c + 1)] for c in ids])


def scene_keys(poses):
    """the keys of the map of the scene's six clouds under ``poses`` at 1.0 m voxels, as a set"""
    s = K.scene()
    return set(M.build_map(s["points"], s["offsets"], poses, voxel_size=1.0)["keys"].tolist())


def face_neighbours(key):
    """the packed keys of the six face neighbours of a packed key (none of the scene's voxels is at the grid's edge)"""
    return [key + sign * (1 << (21 * a)) for a in range(3) for sign in (-1, 1)]


def one_row_of_voxel_three():
    """K.ten_voxels with one row of voxel 3 (exactly min_points rows) named -> (its index, the row as a cloud of one)"""
    pts, off, poses, vox = K.ten_voxels()
    inside = np.nonzero((np.floor(pts) == vox[3]).all(1))[0]
    r = int(inside[-1])
    return r, pts[r:r + 1]


def twelve_voxels_absent_rows():
    """two lattice rows in a voxel no cloud of IK.twelve_voxels reaches"""
    return (np.array([40, 40, 40]) * 64 + np.array([[3, 5, 7], [9, 11, 13]])) / 64.0
