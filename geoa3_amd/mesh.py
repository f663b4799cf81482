"""Triangle meshes as inputs: the OFF / OBJ readers and writers of the reference's Lib/utility.py:229-452, and the
area-weighted surface sampler its Provider/gen_data_mat.py:88-119 defines (sample_points) and never calls -- here for a
ragged batch of meshes in two kernels of libgeoa3_hip.so (mesh_sample.hip), which turns a user's own shapes into the
dense clouds with exact face normals that the re-sampling and the attack consume.

    packed = pack_meshes([read_off(p) for p in paths])
    (pts, nrm), (dense_pts, dense_nrm) = mesh_clouds(packed, 1024, 10000)

The random draws stay the caller's (`u`, `first`), drawn with torch where they are not given.  No CPU path for the
sampler; the readers and writers are plain numpy.

For the mesh attack (geoa3_amd/mesh_attack.py; mesh_attack.hip) the vertices are the variable: to_planar / from_planar,
MeshTopology (edges and CSR, built on the host), and three differentiable operators on planar padded vertices [B,3,Vp] --
surface_points (the points of a FIXED draw at the current vertices), mesh_laplacian_smoothing and mesh_edge_loss
(pytorch3d's, per mesh).

    x, nv = to_planar(packed); topo = MeshTopology.from_packed(packed)
    pts0, nrm0, face_idx, _ = sample_surface(packed, S, u=u)
    loss = f(surface_points(x, nv, packed, face_idx, u)) + mesh_laplacian_smoothing(x, nv, topo).sum()"""
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


# ------------------------------------------------------------------ the mesh attack: vertices as the optimised variable
# (main_attack.py:27-28, 283-293: --attack GeoA3_mesh, which the reference parses and never published.)  The vertices are
# held as the attack loop holds every cloud, planar and padded: verts f32 [B,3,Vp], nv i32 [B]; the faces stay packed.
def to_planar(packed, vp: Optional[int] = None) -> Tuple[Tensor, Tensor]:
    """PackedMeshes -> (verts f32 [B,3,Vp], nv i32 [B]); Vp = the largest vertex count (at least 1) unless given.  Padding
    columns are 0.  Reads vert_off on the host."""
    verts, _, vert_off, _ = packed
    vo = vert_off.cpu().tolist()
    nvs = [vo[i + 1] - vo[i] for i in range(len(vo) - 1)]
    width = max(1, max(nvs)) if vp is None else int(vp)
    if width < max(nvs):
        raise ValueError("vp = %d is smaller than the largest mesh (%d vertices)" % (width, max(nvs)))
    out = verts.new_zeros(len(nvs), 3, width, dtype=torch.float32)
    for b, n in enumerate(nvs):
        if n:
            out[b, :, :n] = verts[vo[b]:vo[b + 1]].t()
    return out, torch.tensor(nvs, dtype=torch.int32, device=verts.device)


def from_planar(verts: Tensor, nv: Tensor, packed) -> PackedMeshes:
    """The inverse of to_planar: the packed batch with its vertices replaced by verts [B,3,Vp] cut to nv (same faces)."""
    counts = nv.cpu().tolist()
    rows = [verts[b, :, :n].t() for b, n in enumerate(counts)]
    out = PackedMeshes(torch.cat(rows).contiguous().float(), packed[1], packed[2], packed[3])
    out.max_faces = getattr(packed, "max_faces", -1)
    return out


class MeshTopology:
    """The fixed topology of a batch, built once on the host from the faces:
        edges    i32 [sumE,2]   the unique undirected edges {i,j}, i < j, local indices, sorted by (i, j); edge_off i64 [B+1]
        row_off  i32 [B Vp + 1] one CSR over the B Vp rows of the padded batch (row b Vp + v; a padding row is empty)
        col      i32 [nnz]      N(v): the neighbours of the row's vertex, local, ASCENDING -- the order every sum runs in
        ne, nv   i32 [B]        E_b and V_b
    A face with an index outside [0,V_b) contributes nothing (the sampler's rule), a face that repeats an index only its
    i != j pairs."""

    def __init__(self, edges, edge_off, row_off, col, ne, nv, vp):
        self.edges, self.edge_off, self.row_off, self.col, self.ne, self.nv, self.vp = edges, edge_off, row_off, col, ne, nv, vp

    @property
    def batch(self) -> int:
        return self.nv.numel()

    @property
    def nnz(self) -> int:
        return self.col.numel()

    @classmethod
    def from_packed(cls, packed, vp: Optional[int] = None) -> "MeshTopology":
        _, faces, vert_off, face_off = packed
        dev = faces.device
        f = faces.cpu().numpy().astype(np.int64).reshape(-1, 3)
        vo, fo = vert_off.cpu().numpy(), face_off.cpu().numpy()
        nvs = np.diff(vo).astype(np.int64)
        b = len(nvs)
        width = max(1, int(nvs.max())) if vp is None else int(vp)
        if width < nvs.max():
            raise ValueError("vp = %d is smaller than the largest mesh (%d vertices)" % (width, nvs.max()))
        if b * (width + 1) > 2 ** 31 - 257:
            raise _lib.Geoa3Error("the padded batch has %d x %d rows, more than the kernels index" % (b, width))
        edges, cols, degs = [], [], np.zeros((b, width), np.int64)
        for i in range(b):
            v = int(nvs[i])
            fb = f[fo[i]:fo[i + 1]]
            fb = fb[((fb >= 0) & (fb < v)).all(1)]
            pairs = np.concatenate([fb[:, [0, 1]], fb[:, [1, 2]], fb[:, [2, 0]]])
            pairs = pairs[pairs[:, 0] != pairs[:, 1]]
            key = np.unique(pairs.min(1) * max(v, 1) + pairs.max(1))       # sorted: by the smaller end, then the larger
            e = np.stack([key // max(v, 1), key % max(v, 1)], 1)
            both = np.concatenate([e, e[:, ::-1]])
            both = both[np.lexsort((both[:, 1], both[:, 0]))]              # rows ascending, neighbours ascending inside
            degs[i] = np.bincount(both[:, 0], minlength=width)
            edges.append(e)
            cols.append(both[:, 1])
        ne = np.array([len(e) for e in edges], np.int64)
        if 2 * ne.sum() >= 2 ** 31:
            raise _lib.Geoa3Error("the batch has %d edges, more than the CSR indexes" % ne.sum())
        row_off = np.concatenate([[0], np.cumsum(degs.reshape(-1))])
        t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a.astype(dt))).to(dev)
        return cls(t(np.concatenate(edges).reshape(-1, 2), np.int32), t(np.concatenate([[0], np.cumsum(ne)]), np.int64),
                   t(row_off, np.int32), t(np.concatenate(cols), np.int32), t(ne, np.int32), t(nvs, np.int32), width)

    def _check(self, verts: Tensor):
        if not verts.is_cuda:
            raise _lib.Geoa3Error("geoa3_amd.mesh has no CPU path: the vertices must be on the GPU")
        if verts.dim() != 3 or tuple(verts.shape) != (self.batch, 3, self.vp):
            raise ValueError("verts must be [B,3,Vp] = %r, not %r" % ((self.batch, 3, self.vp), tuple(verts.shape)))

    def edge_lengths(self, verts: Tensor) -> Tensor:
        """l_ij of every CSR entry, f32 [nnz] (geoa3_mesh_edge_lengths): as target_length of mesh_edge_loss it makes the
        term and its gradient exactly 0 at these vertices."""
        self._check(verts)
        v = verts.detach().contiguous().float()
        out = torch.empty(self.nnz, device=v.device, dtype=torch.float32)
        check(_lib.load().geoa3_mesh_edge_lengths(v.data_ptr(), self.nv.data_ptr(), self.row_off.data_ptr(), _ptr(self.col),
                                                  self.batch, self.vp, self.nnz, _ptr(out), _stream()), "geoa3_mesh_edge_lengths")
        return out


def _faces_of(packed_faces) -> Tuple[Tensor, Tensor]:
    """(faces i32 [sumF,3], face_off i64 [B+1]) of a PackedMeshes, a 4-tuple or the pair itself"""
    if len(packed_faces) == 4:
        return packed_faces[1], packed_faces[3]
    faces, face_off = packed_faces
    return faces, face_off


def _check_draw(verts, nv, faces, face_off, face_idx, u):
    b, vp = verts.shape[0], verts.shape[2]
    if not verts.is_cuda:
        raise _lib.Geoa3Error("geoa3_amd.mesh has no CPU path: the vertices must be on the GPU")
    if verts.dim() != 3 or verts.shape[1] != 3 or nv.numel() != b or face_off.numel() != b + 1:
        raise ValueError("verts must be [B,3,Vp] with nv [B] and face_off [B+1]")
    if face_idx.dim() != 2 or face_idx.shape[0] != b or tuple(u.shape) != (b, face_idx.shape[1], 3):
        raise ValueError("face_idx must be [B,S] and u [B,S,3]")
    if (nv.dtype, faces.dtype, face_off.dtype, face_idx.dtype) != (torch.int32, torch.int32, torch.int64, torch.int32):
        raise TypeError("nv, faces and face_idx are int32, face_off int64")
    return b, vp, int(face_idx.shape[1])


def mesh_points_forward(verts, nv, faces, face_off, face_idx, u) -> Tensor:
    """geoa3_mesh_points: pts f32 [B,3,S] of the draw (face_idx, u) at verts [B,3,Vp].  No autograd (surface_points)."""
    b, vp, s = _check_draw(verts, nv, faces, face_off, face_idx, u)
    v, uu = verts.detach().contiguous().float(), u.detach().contiguous().float()
    pts = torch.empty(b, 3, s, device=v.device, dtype=torch.float32)
    check(_lib.load().geoa3_mesh_points(v.data_ptr(), nv.data_ptr(), _ptr(faces), face_off.data_ptr(),
                                        face_idx.contiguous().data_ptr(), uu.data_ptr(), b, vp, s, faces.shape[0],
                                        pts.data_ptr(), _stream()), "geoa3_mesh_points")
    return pts


def mesh_corner_index(nv, faces, face_off, face_idx, vp: int) -> Tensor:
    """geoa3_mesh_corner_index: i32 [B,3S], entry 3 s + k = the vertex of corner k of sample s (-1: no face)."""
    b, s = face_idx.shape
    corner = torch.empty(b, 3 * s, device=face_idx.device, dtype=torch.int32)
    check(_lib.load().geoa3_mesh_corner_index(nv.data_ptr(), _ptr(faces), face_off.data_ptr(), face_idx.contiguous().data_ptr(),
                                              b, int(vp), s, faces.shape[0], corner.data_ptr(), _stream()),
          "geoa3_mesh_corner_index")
    return corner


def mesh_point_lists(nv, faces, face_off, face_idx, vp: int) -> Tensor:
    """The destination lists of a draw's pullback (every vertex's (sample, corner) entries in ascending order), built ONCE
    per draw: an opaque int32 tensor for mesh_points_backward."""
    b, s = face_idx.shape
    lib = _lib.load()
    nbytes = lib.geoa3_mesh_points_scratch_bytes(b, int(vp), s)
    if nbytes < 0:
        check(int(nbytes), "geoa3_mesh_points_scratch_bytes")
    corner = mesh_corner_index(nv, faces, face_off, face_idx, vp)
    lists = torch.empty(nbytes // 4, device=face_idx.device, dtype=torch.int32)
    check(lib.geoa3_mesh_points_lists(corner.data_ptr(), b, int(vp), s, lists.data_ptr(), _stream()), "geoa3_mesh_points_lists")
    return lists


def mesh_points_backward(g_pts: Tensor, u: Tensor, lists: Tensor, vp: int, out: Optional[Tensor] = None) -> Tensor:
    """geoa3_mesh_points_grad: g_pts [B,3,S] -> g_verts [B,3,Vp], every vertex's float32 products added in ascending
    (sample, corner) order."""
    b, _, s = g_pts.shape
    g, uu = g_pts.detach().contiguous().float(), u.detach().contiguous().float()
    if out is None:
        out = torch.empty(b, 3, int(vp), device=g.device, dtype=torch.float32)
    check(_lib.load().geoa3_mesh_points_grad(g.data_ptr(), uu.data_ptr(), lists.data_ptr(), b, int(vp), s, out.data_ptr(),
                                             _stream()), "geoa3_mesh_points_grad")
    return out


def mesh_reg_forward(verts, nv, row_off, col, ne, target: Optional[Tensor], target_scalar: float):
    """geoa3_mesh_reg -> (lap [B], edge [B], unit [B,4,Vp])"""
    b, _, vp = verts.shape
    if not verts.is_cuda:
        raise _lib.Geoa3Error("geoa3_amd.mesh has no CPU path: the vertices must be on the GPU")
    if target is not None and target.numel() != col.numel():
        raise ValueError("a per-edge target_length holds one value per CSR entry (%d), got %d" % (col.numel(), target.numel()))
    v = verts.detach().contiguous().float()
    lap, edge = (torch.empty(b, device=v.device, dtype=torch.float32) for _ in range(2))
    unit = torch.empty(b, 4, vp, device=v.device, dtype=torch.float32)
    tg = None if target is None else target.detach().contiguous().float()
    check(_lib.load().geoa3_mesh_reg(v.data_ptr(), nv.data_ptr(), row_off.data_ptr(), _ptr(col), ne.data_ptr(),
                                     None if tg is None else _ptr(tg), float(target_scalar), b, vp, col.numel(), 0.0, 0.0,
                                     unit.data_ptr(), lap.data_ptr(), edge.data_ptr(), None, 0, _stream()), "geoa3_mesh_reg")
    return lap, edge, unit


def mesh_reg_backward(verts, nv, row_off, col, ne, target: Optional[Tensor], target_scalar: float, unit: Tensor,
                      g_lap: Optional[Tensor], g_edge: Optional[Tensor], w_lap: float = 1.0, w_edge: float = 1.0,
                      out: Optional[Tensor] = None, add: bool = False) -> Tensor:
    """geoa3_mesh_reg_grad -> g_verts [B,3,Vp] = (add ? out : 0) + w_lap g_lap[b] dLap_b + w_edge g_edge[b] dEdge_b; a
    weight of 0 skips its term (g_lap / g_edge None: ones)."""
    b, _, vp = verts.shape
    v = verts.detach().contiguous().float()
    if out is None:
        if add:
            raise ValueError("add needs the tensor to add to")
        out = torch.empty(b, 3, vp, device=v.device, dtype=torch.float32)
    tg = None if target is None else target.detach().contiguous().float()
    gl = None if g_lap is None else g_lap.detach().contiguous().float()
    ge = None if g_edge is None else g_edge.detach().contiguous().float()
    check(_lib.load().geoa3_mesh_reg_grad(v.data_ptr(), nv.data_ptr(), row_off.data_ptr(), _ptr(col), ne.data_ptr(),
                                          None if tg is None else _ptr(tg), float(target_scalar), unit.data_ptr(),
                                          None if gl is None else gl.data_ptr(), None if ge is None else ge.data_ptr(),
                                          float(w_lap), float(w_edge), b, vp, col.numel(), out.data_ptr(), int(add), _stream()),
          "geoa3_mesh_reg_grad")
    return out


def surface_points(verts: Tensor, nv: Tensor, packed_faces, face_idx: Tensor, u: Tensor, lists: Optional[Tensor] = None) -> Tensor:
    """pytorch3d.ops.sample_points_from_meshes at a FIXED draw: the points [B,3,S] of the draw (face_idx, u) --
    sample_surface's outputs and inputs -- at the current vertices [B,3,Vp]; at the vertices the draw was made on, its
    points bit for bit.  Differentiable in verts (geoa3::mesh_surface_points): the backward is the ordered pullback;
    lists = mesh_point_lists(...) of the draw spares it the sort."""
    from . import library  # noqa: F401  (registers the geoa3:: operators)
    faces, face_off = _faces_of(packed_faces)
    return torch.ops.geoa3.mesh_surface_points(verts, nv, faces, face_off, face_idx, u, lists)


def _reduce(x: Tensor, reduction: Optional[str]) -> Tensor:
    if reduction is None:
        return x
    if reduction != "mean":
        raise ValueError("reduction is None (the per-mesh terms [B]) or 'mean' (pytorch3d's batch value)")
    return x.mean()


def mesh_laplacian_smoothing(verts: Tensor, nv: Tensor, topo: MeshTopology, reduction: Optional[str] = None) -> Tensor:
    """pytorch3d.loss.mesh_laplacian_smoothing(method="uniform") per mesh: Lap_b = (1/V_b) sum_i |mean_{j in N(i)} v_j - v_i|
    -> [B]; reduction="mean": pytorch3d's batch value.  Differentiable in verts, d|x| at 0 taken as 0."""
    from . import library  # noqa: F401
    topo._check(verts)
    return _reduce(torch.ops.geoa3.mesh_reg(verts, nv, topo.row_off, topo.col, topo.ne, None, 0.0)[0], reduction)


def mesh_edge_loss(verts: Tensor, nv: Tensor, topo: MeshTopology, target_length=0.0, reduction: Optional[str] = None) -> Tensor:
    """pytorch3d.loss.mesh_edge_loss per mesh: Edge_b = (1/E_b) sum_{edges} (l_ij - t_ij)^2 -> [B]; target_length a number
    or a tensor with one value per CSR entry (topo.edge_lengths(clean_verts): the clean mesh's own lengths)."""
    from . import library  # noqa: F401
    topo._check(verts)
    per_edge = target_length if isinstance(target_length, torch.Tensor) else None
    scalar = 0.0 if per_edge is not None else float(target_length)
    return _reduce(torch.ops.geoa3.mesh_reg(verts, nv, topo.row_off, topo.col, topo.ne, per_edge, scalar)[1], reduction)
