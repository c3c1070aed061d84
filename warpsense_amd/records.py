"""The record dtypes of the map queries, what takes distance records apart, and the PLY writers."""
from __future__ import annotations

import numpy as np

from . import _lib
from ._lib import WsError

# one record of ws_map_surface: world voxel coordinates and the packed entry (16 bytes)
SURFACE_RECORD = np.dtype([("x", "<i4"), ("y", "<i4"), ("z", "<i4"), ("raw", "<u4")])


# one vertex of ws_map_mesh: world position in millimetres and the smallest corner weight of its cell (16 bytes)
VERT = np.dtype([("x_mm", "<i4"), ("y_mm", "<i4"), ("z_mm", "<i4"), ("weight", "<u4")])


# one record of ws_map_raycast: the hit point and the range along the ray in millimetres; no hit: 0, 0, 0, -1 (16 bytes)
RAY = np.dtype([("x_mm", "<i4"), ("y_mm", "<i4"), ("z_mm", "<i4"), ("range_mm", "<i4")])


# one record of ws_map_sample: the interpolated signed distance in mm, the smallest corner weight of the cell, the class (0 unknown,
# 1 free, 2 surface, 3 inside) and the packed entry of the nearest voxel (16 bytes)
SAMPLE = np.dtype([("d_mm", "<i4"), ("weight", "<i4"), ("cls", "<u4"), ("raw", "<u4")])
SAMPLE_CLASSES = _lib.SAMPLE_CLASSES


def distance_class(rec):
    """The class bits of ws_map_distance records: 2 occupied, 1 free, 0 unknown (uint8)."""
    return (np.asarray(rec, dtype=np.uint32) >> np.uint32(30)).astype(np.uint8)


def distance_d2(rec):
    """The squared distance in voxels of ws_map_distance records (bits 0..23, uint32), clamped at max_dist_vox squared."""
    return np.asarray(rec, dtype=np.uint32) & np.uint32(0xFFFFFF)


def distance_mm(rec, res):
    """The distance of ws_map_distance records in millimetres, res * sqrt(d2) as float32 -- the only float of the route, and it
    is made on the host."""
    return (np.float32(res) * np.sqrt(distance_d2(rec).astype(np.float32))).astype(np.float32)


def write_surface_ply(path, marker):
    """The marker cloud of DeviceMapMemWrapper.surface(marker=True) as a binary little-endian PLY: float x y z (metres) and
    uchar red green blue (the reference's r / g / b in [0, 1) scaled by 255 and truncated)."""
    marker = np.asarray(marker, dtype=np.float32).reshape(-1, 7)
    out = np.empty(len(marker), dtype=np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")]))
    out["x"], out["y"], out["z"] = marker[:, 0], marker[:, 1], marker[:, 2]
    for name, col in (("red", 3), ("green", 4), ("blue", 5)):
        out[name] = np.clip(marker[:, col] * np.float32(255.0), 0.0, 255.0).astype(np.uint8)
    header = ("ply\nformat binary_little_endian 1.0\ncomment warpsense_amd surface cloud\n"
              f"element vertex {len(out)}\nproperty float x\nproperty float y\nproperty float z\n"
              "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n")
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(out.tobytes())
    return len(out)


def write_mesh_ply(path, vertices, faces):
    """The mesh of DeviceMapMemWrapper.mesh() as a binary little-endian PLY: float x y z in metres (mm / 1000.f in single
    precision), faces as a uchar count (3) and int vertex indices.  Returns (vertices, faces) written."""
    vertices = np.asarray(vertices, dtype=VERT).reshape(-1)
    faces = np.asarray(faces, dtype=np.uint32).reshape(-1, 3)
    v = np.empty(len(vertices), dtype=np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4")]))
    for name in "xyz":
        v[name] = vertices[name + "_mm"].astype(np.float32) / np.float32(1000.0)
    f = np.empty(len(faces), dtype=np.dtype([("n", "u1"), ("i", "<i4", (3,))]))
    f["n"] = 3
    f["i"] = faces.astype(np.int32)
    header = ("ply\nformat binary_little_endian 1.0\ncomment warpsense_amd surface-nets mesh\n"
              f"element vertex {len(v)}\nproperty float x\nproperty float y\nproperty float z\n"
              f"element face {len(f)}\nproperty list uchar int vertex_indices\nend_header\n")
    with open(path, "wb") as out:
        out.write(header.encode("ascii"))
        out.write(v.tobytes())
        out.write(f.tobytes())
    return len(v), len(f)


def write_raycast_ply(path, records, gradient=None):
    """The hits of DeviceMapMemWrapper.raycast() (records with range_mm >= 0) as a binary little-endian PLY point cloud: float x y z
    in metres (mm / 1000.f in single precision, as write_mesh_ply) and, when `gradient` is given, float nx ny nz: the gradient
    normalised in float64, then cast (a zero gradient stays zero).  Returns the number of points written."""
    records = np.asarray(records, dtype=RAY).reshape(-1)
    hit = records["range_mm"] >= 0
    names = ["x", "y", "z"] + (["nx", "ny", "nz"] if gradient is not None else [])
    v = np.empty(int(np.count_nonzero(hit)), dtype=np.dtype([(n, "<f4") for n in names]))
    for name in "xyz":
        v[name] = records[name + "_mm"][hit].astype(np.float32) / np.float32(1000.0)
    if gradient is not None:
        g = np.asarray(gradient, dtype=np.int32).reshape(-1, 3)[hit].astype(np.float64)
        length = np.sqrt(np.sum(g * g, axis=1))
        g = g / np.where(length > 0, length, 1.0)[:, None]
        for k, name in enumerate(("nx", "ny", "nz")):
            v[name] = g[:, k].astype(np.float32)
    header = ("ply\nformat binary_little_endian 1.0\ncomment warpsense_amd ray cast\n"
              f"element vertex {len(v)}\n" + "".join(f"property float {n}\n" for n in names) + "end_header\n")
    with open(path, "wb") as out:
        out.write(header.encode("ascii"))
        out.write(v.tobytes())
    return len(v)


# one record of ws_map_frontier: world voxel coordinates and the mask of UNKNOWN neighbours, bits 0..5 = -x +x -y +y -z +z (16 bytes)
FRONTIER_RECORD = np.dtype([("x", "<i4"), ("y", "<i4"), ("z", "<i4"), ("mask", "<u4")])
# one row of its cluster table: record index of the first member, members, bounding box in world voxels, coordinate sums (64 bytes)
FRONTIER_CLUSTER = np.dtype([("first", "<u4"), ("count", "<u4"), ("lo", "<i4", (3,)), ("hi", "<i4", (3,)), ("sum", "<i8", (3,)), ("pad", "<u8")])


def frontier_goals(clusters, resolution, min_size=1):
    """What a planner takes from the cluster table of a frontier call: the clusters of at least min_size voxels, largest first (ties
    by `first`), as (centroids, sizes, lo, hi) -- (k, 3) float64 centroids in metres (sum / count * resolution / 1000), uint32 sizes,
    and the (k, 3) int32 corners of the bounding boxes in world voxels.  Host only: no size filter runs on the device."""
    clusters = np.asarray(clusters, dtype=FRONTIER_CLUSTER).reshape(-1)
    keep = clusters[clusters["count"] >= int(min_size)]
    keep = keep[np.lexsort((keep["first"], -keep["count"].astype(np.int64)))]
    centroid = keep["sum"].astype(np.float64) / keep["count"].astype(np.float64)[:, None] * float(resolution) / 1000.0
    return centroid.reshape(-1, 3), keep["count"].copy(), keep["lo"].copy(), keep["hi"].copy()


def write_frontier_ply(path, records, resolution, labels=None):
    """The records of a frontier call as a binary little-endian PLY point cloud: float x y z in metres (voxel * resolution / 1000 in
    single precision, the point of write_surface_ply), uchar mask and, when `labels` is given, int cluster.  Returns the number of
    points written."""
    records = np.asarray(records, dtype=FRONTIER_RECORD).reshape(-1)
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("mask", "u1")] + ([("cluster", "<i4")] if labels is not None else [])
    v = np.empty(len(records), dtype=np.dtype(fields))
    for name in "xyz":
        v[name] = records[name].astype(np.float32) * np.float32(resolution) / np.float32(1000.0)
    v["mask"] = records["mask"].astype(np.uint8)
    if labels is not None:
        v["cluster"] = np.asarray(labels, dtype=np.uint32).reshape(-1).astype(np.int32)
    header = ("ply\nformat binary_little_endian 1.0\ncomment warpsense_amd frontier\n"
              f"element vertex {len(v)}\nproperty float x\nproperty float y\nproperty float z\nproperty uchar mask\n"
              + ("property int cluster\n" if labels is not None else "") + "end_header\n")
    with open(path, "wb") as out:
        out.write(header.encode("ascii"))
        out.write(v.tobytes())
    return len(v)


# ws_map_reach_paths: the header of a goal (status 0 reached, 1 not reachable, 2 outside the box) and one record of its path, 16 bytes each
REACH_PATH_HEADER = np.dtype([("cost", "<u4"), ("steps", "<u4"), ("written", "<u4"), ("status", "<u4")])
REACH_PATH_RECORD = np.dtype([("x", "<i4"), ("y", "<i4"), ("z", "<i4"), ("cost", "<u4")])
REACH_UNREACHABLE = _lib.WS_REACH_UNREACHABLE


def reach_mm(cost, resolution):
    """The path length in millimetres that a cost of ws_map_reach stands for: cost * resolution / 10 (a face step weighs 10) as float64;
    an unreachable cost becomes inf."""
    cost = np.asarray(cost, dtype=np.uint32)
    return np.where(cost == np.uint32(REACH_UNREACHABLE), np.inf, cost.astype(np.float64) * float(resolution) / 10.0)


def write_path_ply(path, headers, records, resolution):
    """The paths of reach_paths as a binary little-endian PLY: the written records of every reached goal as vertices (float x y z in
    metres, voxel * resolution / 1000 in single precision, int path, uint cost) and an edge between consecutive records of a path.
    Returns (vertices, edges) written."""
    headers = np.asarray(headers, dtype=REACH_PATH_HEADER).reshape(-1)
    records = np.asarray(records, dtype=REACH_PATH_RECORD).reshape(len(headers), -1)
    rows = [records[i, :int(h["written"])] for i, h in enumerate(headers)]
    n = sum(len(r) for r in rows)
    v = np.empty(n, dtype=np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("path", "<i4"), ("cost", "<u4")]))
    e = np.empty(sum(max(len(r) - 1, 0) for r in rows), dtype=np.dtype([("vertex1", "<i4"), ("vertex2", "<i4")]))
    at = ae = 0
    for i, r in enumerate(rows):
        for name in "xyz":
            v[name][at:at + len(r)] = r[name].astype(np.float32) * np.float32(resolution) / np.float32(1000.0)
        v["path"][at:at + len(r)], v["cost"][at:at + len(r)] = i, r["cost"]
        k = max(len(r) - 1, 0)
        e["vertex1"][ae:ae + k], e["vertex2"][ae:ae + k] = np.arange(at, at + k), np.arange(at + 1, at + 1 + k)
        at, ae = at + len(r), ae + k
    header = ("ply\nformat binary_little_endian 1.0\ncomment warpsense_amd reach paths\n"
              f"element vertex {len(v)}\nproperty float x\nproperty float y\nproperty float z\nproperty int path\nproperty uint cost\n"
              f"element edge {len(e)}\nproperty int vertex1\nproperty int vertex2\nend_header\n")
    with open(path, "wb") as out:
        out.write(header.encode("ascii"))
        out.write(v.tobytes())
        out.write(e.tobytes())
    return len(v), len(e)


# one record of ws_map_view_gain per view (32 bytes), and with WS_GAIN_RAYS one per (view, ray), view-major (8 bytes): stop is the k of
# the blocking sample, -1 for none, -2 for a dead ray
VIEW_GAIN_RECORD = np.dtype([("unknown_k2", "<u8"), ("free_k2", "<u8"), ("unknown", "<u4"), ("free", "<u4"), ("blocked", "<u4"), ("live", "<u4")])
VIEW_GAIN_RAY = np.dtype([("unknown", "<u4"), ("stop", "<i4")])


def view_fan(rings, azimuths, v_fov_deg):
    """The fan of a view-gain call: rings x azimuths directions, elevations spread evenly over v_fov_deg around the horizon (one ring:
    the horizon), azimuths evenly around the circle, ring-major.  Integers by the scaling of TSDFMapping.raycast_rays: the largest
    component is 2^20 in magnitude, rounded to nearest, so no direction is zero.  Returns (rings * azimuths, 3) int32."""
    rings, azimuths = int(rings), int(azimuths)
    if rings < 1 or azimuths < 1:
        raise WsError("view_fan: rings and azimuths must be at least 1")
    el = np.deg2rad(np.linspace(-0.5, 0.5, rings) * float(v_fov_deg)) if rings > 1 else np.zeros(1)
    az = 2.0 * np.pi * np.arange(azimuths, dtype=np.float64) / azimuths
    d = np.stack([np.cos(el)[:, None] * np.cos(az)[None, :], np.cos(el)[:, None] * np.sin(az)[None, :],
                  np.sin(el)[:, None] * np.ones(azimuths)[None, :]], axis=-1).reshape(-1, 3)
    d = d * (float(1 << 20) / np.max(np.abs(d), axis=1))[:, None]
    return np.rint(d).astype(np.int32)


def gain_volume_m3(records, resolution, solid_angle_per_ray):
    """The unknown volume in cubic metres that the views of a view-gain call would see: unknown_k2 * step^3 * solid_angle_per_ray with
    step = max(resolution / 2, 1) mm (a sample at range k step stands for (k step)^2 step of volume per steradian), as float64."""
    records = np.asarray(records, dtype=VIEW_GAIN_RECORD).reshape(-1)
    step_m = max(int(resolution) // 2, 1) / 1000.0
    return records["unknown_k2"].astype(np.float64) * step_m ** 3 * float(solid_angle_per_ray)


def rank_views(records, cost, resolution, lam_per_m):
    """Rank the views of a view-gain call by what they show against what the way there costs: score = unknown_k2 * exp(-lam_per_m *
    reach_mm(cost) / 1000) in float64 on the host; an unreachable view (cost 0xFFFFFFFF) scores -inf.  Returns (order, score): the view
    indices by descending score, ties to the lower index."""
    records = np.asarray(records, dtype=VIEW_GAIN_RECORD).reshape(-1)
    mm = reach_mm(np.asarray(cost, dtype=np.uint32).reshape(-1), resolution)
    if len(mm) != len(records):
        raise WsError("rank_views: one cost per view")
    with np.errstate(invalid="ignore"):
        score = np.where(np.isinf(mm), -np.inf, records["unknown_k2"].astype(np.float64) * np.exp(-float(lam_per_m) * np.where(np.isinf(mm), 0.0, mm) / 1000.0))
    return np.argsort(-score, kind="stable"), score
