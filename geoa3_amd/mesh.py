"""Triangle meshes as inputs: the OFF / OBJ readers and writers of the reference's Lib/utility.py:229-452, and the
area-weighted surface sampler its Provider/gen_data_mat.py:88-119 defines (sample_points) and never calls -- here for a
ragged batch of meshes in two kernels of libgeoa3_hip.so (mesh_sample.hip), which turns a user's own shapes into the
dense clouds with exact face normals that the re-sampling and the attack consume.

    packed = pack_meshes([read_off(p) for p in paths])
    (pts, nrm), (dense_pts, dense_nrm) = mesh_clouds(packed, 1024, 10000)

The random draws stay the caller's (`u`, `first`), drawn with torch where they are not given.  No CPU path for the
sampler; the readers and writers are plain numpy."""
from __future__ import annotations

from typing import NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import check

Tensor = torch.Tensor

MAX_FACES_PER_MESH = 1 << 22      # a mesh's integer area total stays below 2^62
MAX_SURFACE_SAMPLES = 16384       # the point limit of geoa3_fps_sample, which mesh_clouds feeds


class MeshFormatError(ValueError):
    pass


# ------------------------------------------------------------------ readers and writers (Lib/utility.py:229-452)
def _content_lines(path):
    with open(path, "r") as fp:
        return [ln.strip() for ln in fp]


def read_off(path) -> Tuple[np.ndarray, np.ndarray]:
    """Lib/utility.py:375-452: an OFF (or COFF) file -> (vertices f32 [V,3], faces i32 [F,3]).  Accepts ModelNet's broken
    first line that holds the counts too (`OFF8 12 0`), and vertex rows with more than three columns (the colours of
    COFF), of which the first three are kept.  A face that is not a triangle is rejected.  Blank lines and `#` comments
    are passed over.  Vertex indices are NOT checked against V here: the table kernel counts such faces as bad."""
    lines = [ln for ln in _content_lines(path) if ln and not ln.startswith("#")]
    if not lines:
        raise MeshFormatError("%s: empty file" % path)
    head = lines[0]
    if head[:4].upper() == "COFF":
        rest = head[4:]
    elif head[:3].upper() == "OFF":
        rest = head[3:]
    else:
        raise MeshFormatError("%s: not an OFF file (first line %r)" % (path, head))
    at = 1
    counts = rest.split()
    if not counts:                 # the regular case: the counts are on the next line
        if len(lines) < 2:
            raise MeshFormatError("%s: no counts line" % path)
        counts, at = lines[1].split(), 2
    if len(counts) != 3:
        raise MeshFormatError("%s: the counts line must read `V F E`, got %r" % (path, " ".join(counts)))
    nv, nf = int(counts[0]), int(counts[1])
    if nv <= 0 or nf <= 0:
        raise MeshFormatError("%s: %d vertices and %d faces" % (path, nv, nf))
    if len(lines) < at + nv + nf:
        raise MeshFormatError("%s: %d vertices and %d faces announced, %d rows present" % (path, nv, nf, len(lines) - at))
    verts = np.empty((nv, 3), np.float32)
    for i in range(nv):
        row = lines[at + i].split()
        if len(row) < 3:
            raise MeshFormatError("%s: vertex %d has %d columns" % (path, i, len(row)))
        verts[i] = [float(x) for x in row[:3]]
    faces = np.empty((nf, 3), np.int32)
    for i in range(nf):
        row = lines[at + nv + i].split()
        n = int(row[0])
        if n != 3:
            raise MeshFormatError("%s: face %d has %d vertices, only triangles are supported" % (path, i, n))
        if len(row) < 4:
            raise MeshFormatError("%s: face %d announces 3 vertices and lists %d" % (path, i, len(row) - 1))
        faces[i] = [int(x) for x in row[1:4]]     # (COFF may append a colour to the row)
    return verts, faces


def read_obj(path) -> Tuple[np.ndarray, np.ndarray]:
    """Lib/utility.py:267-333: an OBJ file -> (vertices f32 [V,3], faces i32 [F,3]).  `v x y z [nx ny nz]` and
    `f a b c` with a = v, v/vt, v//vn or v/vt/vn, 1-based; a face that repeats a vertex is skipped, a face that is not a
    triangle rejected; every other record (vn, vt, g, usemtl ...) is passed over."""
    verts, faces = [], []
    for ln in _content_lines(path):
        parts = ln.split()
        if not parts:
            continue
        if parts[0] == "v":
            if len(parts) not in (4, 7):
                raise MeshFormatError("%s: a vertex reads `v x y z` or `v x y z nx ny nz`, got %r" % (path, ln))
            verts.append([float(x) for x in parts[1:4]])
        elif parts[0] == "f":
            if len(parts) != 4:
                raise MeshFormatError("%s: face %r has %d vertices, only triangles are supported" % (path, ln, len(parts) - 1))
            idx = []
            for comp in parts[1:]:
                fields = comp.split("/")
                if not 1 <= len(fields) <= 3 or not fields[0]:
                    raise MeshFormatError("%s: face component %r is not v, v/vt or v/vt/vn" % (path, comp))
                idx.append(int(fields[0]) - 1)
            if len(set(idx)) == 3:
                faces.append(idx)
    return (np.asarray(verts, np.float32).reshape(-1, 3), np.asarray(faces, np.int32).reshape(-1, 3))


def _checked(path, vertices, faces):
    vertices, faces = np.asarray(vertices), np.asarray(faces)
    if vertices.ndim != 2 or vertices.shape[1] != 3 or len(vertices) == 0:
        raise MeshFormatError("%s: vertices must be [V,3] with V > 0" % path)
    if faces.ndim != 2 or faces.shape[1] != 3 or len(faces) == 0:
        raise MeshFormatError("%s: faces must be [F,3] with F > 0, only triangles are supported" % path)
    if faces.min() < 0 or faces.max() >= len(vertices):
        raise MeshFormatError("%s: a face names a vertex outside [0, %d)" % (path, len(vertices)))
    return vertices, faces


def write_off(path, vertices, faces) -> None:
    """Lib/utility.py:335-373, faces [F,3] (the leading 3 of every row is written here).  Coordinates are written with
    repr, so a float32 array reads back to the same bits."""
    vertices, faces = _checked(path, vertices, faces)
    with open(path, "w") as fp:
        fp.write("OFF\n%d %d 0\n" % (len(vertices), len(faces)))
        for v in vertices.tolist():
            fp.write("%r %r %r\n" % tuple(v))
        for f in faces.tolist():
            fp.write("3 %d %d %d\n" % tuple(f))


def write_obj(path, vertices, faces) -> None:
    """Lib/utility.py:229-265: `v x y z` and 1-based `f a b c`."""
    vertices, faces = _checked(path, vertices, faces)
    with open(path, "w") as fp:
        for v in vertices.tolist():
            fp.write("v %r %r %r\n" % tuple(v))
        for f in faces.tolist():
            fp.write("f %d %d %d\n" % (f[0] + 1, f[1] + 1, f[2] + 1))


READERS = {".off": read_off, ".obj": read_obj}


# ------------------------------------------------------------------ the batch
class _Packed(NamedTuple):
    verts: Tensor
    faces: Tensor
    vert_off: Tensor
    face_off: Tensor


class PackedMeshes(_Packed):
    """A ragged batch on the device, a 4-tuple: verts f32 [sumV,3], faces i32 [sumF,3] (indices local to their mesh),
    vert_off and face_off i64 [B+1].  max_faces (an attribute beside the tuple): the largest face count of one mesh when
    the packing knows it on the host, else -1 (it is then read back from face_off)."""
    max_faces = -1

    @property
    def batch(self) -> int:
        return self.vert_off.numel() - 1


def pack_meshes(meshes: Sequence[Tuple[np.ndarray, np.ndarray]], device="cuda") -> PackedMeshes:
    """[(verts [V,3], faces [F,3]), ...] -> PackedMeshes on `device`.  A mesh may be empty (no faces, no vertices)."""
    if len(meshes) == 0:
        raise ValueError("pack_meshes needs at least one mesh")
    vs = [np.ascontiguousarray(np.asarray(v, np.float32).reshape(-1, 3)) for v, _ in meshes]
    fs = [np.ascontiguousarray(np.asarray(f, np.int32).reshape(-1, 3)) for _, f in meshes]
    nf = [len(f) for f in fs]
    if max(nf) > MAX_FACES_PER_MESH or sum(nf) >= 1 << 31:
        raise _lib.Geoa3Error("a mesh may hold at most 2^22 faces and a batch fewer than 2^31, got max %d, sum %d"
                              % (max(nf), sum(nf)))
    vert_off = np.concatenate([[0], np.cumsum([len(v) for v in vs])]).astype(np.int64)
    face_off = np.concatenate([[0], np.cumsum(nf)]).astype(np.int64)
    dev = torch.device(device)
    packed = PackedMeshes(torch.from_numpy(np.concatenate(vs)).to(dev), torch.from_numpy(np.concatenate(fs)).to(dev),
                          torch.from_numpy(vert_off).to(dev), torch.from_numpy(face_off).to(dev))
    packed.max_faces = int(max(nf))
    return packed


def _unpack(packed):
    """(PackedMeshes, B, total_verts, total_faces, max_faces) of a PackedMeshes or a plain 4-tuple (whose largest face
    count is then read back from the device)."""
    max_faces = getattr(packed, "max_faces", -1)
    verts, faces, vert_off, face_off = packed
    for t in (verts, faces, vert_off, face_off):
        if not t.is_cuda:
            raise _lib.Geoa3Error("geoa3_amd.mesh has no CPU path: pack the meshes onto the GPU")
    if (verts.dtype, faces.dtype, vert_off.dtype, face_off.dtype) != (torch.float32, torch.int32, torch.int64, torch.int64):
        raise TypeError("packed meshes are (f32 verts, i32 faces, i64 vert_off, i64 face_off)")
    if verts.dim() != 2 or verts.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError("verts must be [sumV,3] and faces [sumF,3]")
    b = face_off.numel() - 1
    if b < 1 or vert_off.numel() != b + 1:
        raise ValueError("vert_off and face_off must both hold B+1 >= 2 offsets")
    if max_faces < 0:
        max_faces = int((face_off[1:] - face_off[:-1]).max().item())
    packed = PackedMeshes(verts.contiguous(), faces.contiguous(), vert_off.contiguous(), face_off.contiguous())
    packed.max_faces = max_faces
    return packed, b, verts.shape[0], faces.shape[0], max_faces


def _ptr(t: Tensor):
    return t.data_ptr() if t.numel() else None


def _stream():
    return torch.cuda.current_stream().cuda_stream


def area_table(packed) -> Tuple[Tensor, Tensor]:
    """-> (table [sumF], bad_faces int32 [B]): per mesh the inclusive prefix sum of the integer face weights
    (geoa3_mesh_area_table).  The 64-bit unsigned prefixes stay below 2^62 and are held in an int64 tensor."""
    packed, b, tv, tf, mf = _unpack(packed)
    lib = _lib.load()
    nbytes = lib.geoa3_mesh_table_bytes(tf)
    if nbytes < 0:
        check(int(nbytes), "geoa3_mesh_table_bytes")
    table = torch.empty(nbytes // 8, device=packed.verts.device, dtype=torch.int64)
    bad = torch.empty(b, device=packed.verts.device, dtype=torch.int32)
    check(lib.geoa3_mesh_area_table(_ptr(packed.verts), _ptr(packed.faces), packed.vert_off.data_ptr(),
                                    packed.face_off.data_ptr(), b, tv, tf, mf, _ptr(table), bad.data_ptr(), _stream()),
          "geoa3_mesh_area_table")
    return table, bad


def sample_surface(packed, num_samples: int, u: Optional[Tensor] = None, generator: Optional[torch.Generator] = None):
    """gen_data_mat.py:88-119 for a batch: -> (points [B,3,S], normals [B,3,S], face_idx int32 [B,S], bad_faces int32
    [B]).  A face is picked with probability proportional to its area, the point is uniform on it, the normal is the
    face's own (unit, signed by the winding).  u [B,S,3] in [0,1): the three draws of every sample (default:
    torch.rand on the device, from `generator` when given).  A mesh without any area comes out NaN with face_idx -1."""
    packed, b, tv, tf, mf = _unpack(packed)
    dev = packed.verts.device
    s = int(num_samples)
    if s < 1:
        raise ValueError("num_samples must be positive")
    if u is None:
        u = torch.rand(b, s, 3, device=dev, dtype=torch.float32, generator=generator)
    elif tuple(u.shape) != (b, s, 3):
        raise ValueError("u must be [B,S,3] = %r, not %r" % ((b, s, 3), tuple(u.shape)))
    u = u.to(device=dev, dtype=torch.float32).contiguous()
    table, bad = area_table(packed)
    pts = torch.empty(b, 3, s, device=dev, dtype=torch.float32)
    nrm = torch.empty(b, 3, s, device=dev, dtype=torch.float32)
    fidx = torch.empty(b, s, device=dev, dtype=torch.int32)
    check(_lib.load().geoa3_mesh_sample(_ptr(packed.verts), _ptr(packed.faces), packed.vert_off.data_ptr(),
                                        packed.face_off.data_ptr(), _ptr(table), u.data_ptr(), b, s, tv, tf, mf,
                                        pts.data_ptr(), nrm.data_ptr(), fidx.data_ptr(), _stream()), "geoa3_mesh_sample")
    return pts, nrm, fidx, bad


def mesh_clouds(packed, npoint: int, dense_npoints: int, surface_samples: int = MAX_SURFACE_SAMPLES, first=None, u=None,
                generator: Optional[torch.Generator] = None, return_bad_faces: bool = False):
    """Meshes -> the two clouds Provider/gen_data_mat.py writes: `surface_samples` surface points per mesh (at most
    16384, what the farthest-point sampler takes), then utility.farthest_points_normalized to npoint and, separately,
    to dense_npoints points, each centred and scaled by its own statistics as gen_data_mat.py:195-197 does.
    -> ((points [B,3,npoint], normals), (dense points [B,3,dense_npoints], dense normals)); the second pair is None when
    dense_npoints <= 0.  first: the farthest-point sampler's first index, [B] for both or a pair ([B], [B]) (default:
    drawn per call as the reference draws np.random.randint per call).  With return_bad_faces also bad_faces [B]."""
    from . import utility as U
    s = int(surface_samples)
    if not 1 <= s <= MAX_SURFACE_SAMPLES:
        raise _lib.Geoa3Error("surface_samples must lie in 1 .. %d (the farthest-point sampler's limit), got %d"
                              % (MAX_SURFACE_SAMPLES, s))
    if max(npoint, dense_npoints) > s or npoint < 1:
        raise ValueError("npoint (>= 1) and dense_npoints may not exceed surface_samples = %d" % s)
    pts, nrm, _, bad = sample_surface(packed, s, u, generator)
    firsts = tuple(first) if isinstance(first, (tuple, list)) else (first, first)
    small = U.farthest_points_normalized(pts, nrm, int(npoint), firsts[0])
    dense = U.farthest_points_normalized(pts, nrm, int(dense_npoints), firsts[1]) if dense_npoints > 0 else None
    return (small, dense, bad) if return_bad_faces else (small, dense)
