"""Golden vectors of the reference's ``points3D`` readers: writes a small authored COLMAP point model in both flavours
(tests/golden/colmap_points/{bin,txt}/points3D.*, with ``struct`` / ``%r``, following the published COLMAP file layout), has
the REFERENCE's readers (splat/read_colmap.py:242-309) parse them, and stores what they returned as
tests/golden/colmap_points.npz -- the fixture our own readers (colmap.read_points3D_*) are held to, field for field.

Needs a checkout of the reference (dcaustin33/intro_to_gaussian_splatting) where oracle/capture_golden.py looks for it; it is
imported through that script's own importer and never copied -- this script writes data only.

The model: 40 points in the box [-1, 1]^3 (in front of a camera a few units back along -z), ids that are neither consecutive
nor in ascending order in the file, tracks 1 to 5 long over the images 1..3 (eight points have a track of one: what
``Gaussians.from_colmap_points(min_track_length=2)`` filters).

    python tools/capture_points3d_golden.py
"""
from __future__ import annotations

import os
import struct
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT_DIR = os.path.join(ROOT, "tests", "golden")


def authored_points():
    """[(id, xyz, rgb, error, [(image_id, point2D_idx), ...])], in FILE order."""
    rs = np.random.RandomState(77)
    ids = rs.permutation(np.arange(3, 3 + 7 * 40, 7))           # 40 ids, stride 7, shuffled
    pts = []
    for k, pid in enumerate(ids):
        length = 1 if k % 5 == 0 else int(rs.randint(2, 6))
        track = [(int(rs.randint(1, 4)), int(rs.randint(0, 2000))) for _ in range(length)]
        pts.append((int(pid), rs.uniform(-1.0, 1.0, 3), rs.randint(0, 256, 3), float(rs.uniform(0.05, 2.0)), track))
    return pts


def write_model(out_dir: str, pts) -> None:
    os.makedirs(os.path.join(out_dir, "bin"), exist_ok=True)
    os.makedirs(os.path.join(out_dir, "txt"), exist_ok=True)
    with open(os.path.join(out_dir, "bin", "points3D.bin"), "wb") as f:
        f.write(struct.pack("<Q", len(pts)))
        for pid, xyz, rgb, err, track in pts:
            f.write(struct.pack("<QdddBBBd", pid, *[float(v) for v in xyz], *[int(v) for v in rgb], err))
            f.write(struct.pack("<Q", len(track)))
            for image_id, idx in track:
                f.write(struct.pack("<ii", image_id, idx))
    with open(os.path.join(out_dir, "txt", "points3D.txt"), "w") as f:
        f.write("# 3D point list with one line of data per point:\n")
        f.write("#   POINT3D_ID, X, Y, Z, R, G, B, ERROR, TRACK[] as (IMAGE_ID, POINT2D_IDX)\n")
        for pid, xyz, rgb, err, track in pts:
            f.write("%d %s %s %r %s\n" % (pid, " ".join(repr(float(v)) for v in xyz), " ".join("%d" % int(v) for v in rgb), err,
                                          " ".join("%d %d" % t for t in track)))


def main() -> None:
    sys.path.insert(0, ROOT)
    from oracle import capture_golden          # its importer: stubs plyfile, puts the reference on the path

    capture_golden._import_reference()
    from splat import read_colmap as rc

    pts = authored_points()
    out_dir = os.path.join(OUT_DIR, "colmap_points")
    write_model(out_dir, pts)
    parsed = {}
    for flavour, reader in (("bin", rc.read_points3D_binary), ("txt", rc.read_points3D_text)):
        points = reader(os.path.join(out_dir, flavour, "points3D." + flavour))
        parsed[flavour + "_ids"] = np.array(list(points), dtype=np.int64)           # in the reader's (= the file's) order
        for pid, p in points.items():
            assert p.id == pid
            parsed["%s_pt%d_xyz" % (flavour, pid)] = np.asarray(p.xyz, dtype=np.float64)
            parsed["%s_pt%d_rgb" % (flavour, pid)] = np.asarray(p.rgb, dtype=np.int64)
            parsed["%s_pt%d_error" % (flavour, pid)] = np.float64(p.error)
            parsed["%s_pt%d_image_ids" % (flavour, pid)] = np.asarray(p.image_ids, dtype=np.int64)
            parsed["%s_pt%d_point2D_idxs" % (flavour, pid)] = np.asarray(p.point2D_idxs, dtype=np.int64)
    path = os.path.join(OUT_DIR, "colmap_points.npz")
    np.savez_compressed(path, **parsed)
    lengths = [len(t[4]) for t in pts]
    print("colmap_points: %d points, tracks %d..%d, both flavours parsed by the reference -> %s (%.0f KB)" % (
        len(pts), min(lengths), max(lengths), path, os.path.getsize(path) / 1e3))


if __name__ == "__main__":
    main()
