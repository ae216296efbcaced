"""Tensor-level wrapper over the sparse 3-D convolution of csrc/spconv.hip (include/lidarcrafter_hip.h: lc_spconv_*).
Like ops.py: CUDA(HIP) tensors only, no CPU / eager-PyTorch fallback.

A sparse tensor at stride s is rows F [N, C] over coordinates [N, 4] int32 = (x, y, z, batch) whose spatial entries are
multiples of s (not divided by it).  `CoordLevels` holds the five coordinate levels of one input and builds every
neighbour table once: `same(l)` [N_l, 27], `down(l)` [N_{l+1}, 8] and `up(l)` [N_l, 8] (from level l + 1)."""
from __future__ import annotations

from typing import Optional

import torch

from ._lib import check, lib
from .ops import _F32, _entry, _req, _stream

TILE = 64                      # output rows per block of the convolution kernel (csrc/spconv.hip SP_T = LC_SPCONV_TILE)
MAX_COORD = 262143             # include/lidarcrafter_hip.h LC_SPCONV_MAX_COORD (tests/test_spconv_host.py compares)
MAX_BATCH = 510                # LC_SPCONV_MAX_BATCH: the packed key stays a non-negative int64
WIDTHS_IN = (4, 16, 32, 48, 64, 96, 128, 192)
WIDTHS_OUT = (16, 32, 48, 64, 128)
KIND_SAME, KIND_DOWN, KIND_UP = 0, 1, 2
_I32 = torch.int32


def _req_coords(c: torch.Tensor, name: str) -> None:
    if not isinstance(c, torch.Tensor) or not c.is_cuda:
        raise RuntimeError(f"lidarcrafter_amd.ops_spconv: `{name}` must be a CUDA(HIP) tensor -- no CPU fallback on the "
                           "hot path")
    if c.dtype != _I32 or c.dim() != 2 or c.shape[1] != 4 or not c.is_contiguous() or c.shape[0] < 1:
        raise ValueError(f"`{name}` must be contiguous int32 [N >= 1, 4] = (x, y, z, batch), got {c.dtype} "
                         f"{tuple(c.shape)}")


def pack_keys(coords: torch.Tensor) -> torch.Tensor:
    """int64 key batch << 54 | x << 36 | y << 18 | z of every row: ascending keys = ascending (batch, x, y, z)."""
    c = coords.to(torch.int64)
    return (c[:, 3] << 54) | (c[:, 0] << 36) | (c[:, 1] << 18) | c[:, 2]


def unpack_keys(keys: torch.Tensor) -> torch.Tensor:
    m = (1 << 18) - 1
    return torch.stack([(keys >> 36) & m, (keys >> 18) & m, keys & m, keys >> 54], dim=1).to(_I32).contiguous()


def downsample_coords(coords: torch.Tensor, stride: int) -> torch.Tensor:
    """The coordinates of a ks 2 / stride 2 convolution's output: the unique rows of (xyz // 2s) * 2s with their batch,
    ascending by (batch, x, y, z) (a sort of the packed keys: plumbing)."""
    s2 = 2 * int(stride)
    c = coords.clone()
    c[:, :3] = torch.div(c[:, :3], s2, rounding_mode="floor") * s2
    return unpack_keys(torch.unique(pack_keys(c), sorted=True))


@_entry
def hash_build(coords: torch.Tensor, max_coord: int, n_batch: int) -> torch.Tensor:
    """The coordinate hash of `coords` (a uint8 device buffer the map kernels read).  `max_coord`, `n_batch`: the largest
    spatial entry and the number of clouds, stated by the caller (the limits are checked on the host, before a launch)."""
    _req_coords(coords, "coords")
    n = coords.shape[0]
    nbytes = int(lib().lc_spconv_hash_bytes(n))
    if nbytes <= 0:
        raise ValueError(f"hash_build: {n} rows are outside what the table takes")
    table = torch.empty(nbytes // 8, device=coords.device, dtype=torch.int64)
    check(lib().lc_spconv_hash_build(coords.data_ptr(), n, int(max_coord), int(n_batch), table.data_ptr(), nbytes,
                                     _stream()), "lc_spconv_hash_build")
    return table


@_entry
def kernel_map(coords: torch.Tensor, kind: int, stride: int, table: torch.Tensor, n_table: int) -> torch.Tensor:
    """nbr [M, 27 | 8] int32: for every row of `coords` the row of `table` at coords + offset_k, -1 when absent."""
    _req_coords(coords, "coords")
    if kind not in (KIND_SAME, KIND_DOWN, KIND_UP):
        raise ValueError(f"kernel_map: kind {kind}")
    if not table.is_cuda or table.dtype != torch.int64 or table.numel() * 8 < int(lib().lc_spconv_hash_bytes(n_table)):
        raise ValueError("kernel_map: `table` is not the hash_build of `n_table` rows")
    m = coords.shape[0]
    nbr = torch.empty((m, 27 if kind == KIND_SAME else 8), device=coords.device, dtype=_I32)
    check(lib().lc_spconv_map(coords.data_ptr(), m, kind, int(stride), table.data_ptr(), int(n_table), nbr.data_ptr(),
                              _stream()), "lc_spconv_map")
    return nbr


def _rows(t: torch.Tensor, name: str, who: str = "sparse_conv"):
    _req(t, name)
    if t.dim() != 2 or t.stride(1) != 1 or t.shape[0] < 1:
        raise ValueError(f"{who}: `{name}` must be [N, C] rows with unit column stride, got {tuple(t.shape)} "
                         f"strides {t.stride()}")
    return t.stride(0) if t.shape[0] > 1 else max(t.stride(0), t.shape[1])


@_entry
def sparse_conv(x: torch.Tensor, nbr: Optional[torch.Tensor], w: torch.Tensor, b: Optional[torch.Tensor] = None,
                residual: Optional[torch.Tensor] = None, relu: bool = False, out: Optional[torch.Tensor] = None,
                out_col: int = 0) -> torch.Tensor:
    """out[j, out_col : out_col + Co] = act(sum_k x[nbr[j, k], :] @ w[k] + b + residual[j]).  x [N, Ci] rows (a column
    slice of a wider buffer is fine); nbr [M, K] int32 with -1 for absent, None with w [1, Ci, Co]: the dense product;
    w [K, Ci, Co] contiguous; residual [M, Co] rows; `out` [M, >= out_col + Co] row-major, the other columns are left as
    they are.  Returns `out`."""
    ldx = _rows(x, "x")
    _req(w, "w")
    if w.dim() != 3 or not w.is_contiguous() or w.shape[1] != x.shape[1]:
        raise ValueError(f"sparse_conv: `w` must be contiguous [K, {x.shape[1]}, Co], got {tuple(w.shape)}")
    K, Ci, Co = w.shape
    if nbr is None:
        if K != 1:
            raise ValueError("sparse_conv: a kernel of more than one offset needs its neighbour table")
        M = x.shape[0]
    else:
        if not nbr.is_cuda or nbr.dtype != _I32 or nbr.dim() != 2 or not nbr.is_contiguous() or nbr.shape[1] != K:
            raise ValueError(f"sparse_conv: `nbr` must be contiguous int32 [M, {K}]")
        M = nbr.shape[0]
    if b is not None:
        _req(b, "b")
        if tuple(b.shape) != (Co,) or not b.is_contiguous():
            raise ValueError(f"sparse_conv: `b` must be contiguous [{Co}]")
    ldr = 0
    if residual is not None:
        ldr = _rows(residual, "residual")
        if tuple(residual.shape) != (M, Co):
            raise ValueError(f"sparse_conv: `residual` must be [{M}, {Co}], got {tuple(residual.shape)}")
    if out is None:
        out = torch.empty((M, out_col + Co), device=x.device, dtype=_F32)
    ldy = _rows(out, "out")
    if out.shape[0] != M or out.shape[1] < out_col + Co or out_col < 0:
        raise ValueError(f"sparse_conv: `out` must be [{M}, >= {out_col + Co}], got {tuple(out.shape)}")
    check(lib().lc_spconv_fwd(x.data_ptr(), ldx, None if nbr is None else nbr.data_ptr(), x.shape[0], w.data_ptr(),
                              None if b is None else b.data_ptr(), None if residual is None else residual.data_ptr(),
                              ldr, out.data_ptr(), ldy, int(out_col), M, Ci, Co, K, 1 if relu else 0, _stream()),
          "lc_spconv_fwd")
    return out


@_entry
def sector_means(feats: torch.Tensor, coords: torch.Tensor, offsets: torch.Tensor, edges: torch.Tensor,
                 voxel: float) -> torch.Tensor:
    """[n_clouds, 16 C]: per cloud (rows offsets[c] .. offsets[c + 1]) and depth sector the mean feature row; d = |xyz -
    mean xyz| * voxel against `edges` (device float32 [17]); an empty sector gives zeros."""
    ldf = _rows(feats, "feats")
    _req_coords(coords, "coords")
    _req(edges, "edges")
    if coords.shape[0] != feats.shape[0] or tuple(edges.shape) != (17,) or not edges.is_contiguous():
        raise ValueError("sector_means: coords / feats rows differ, or `edges` is not contiguous [17]")
    if not offsets.is_cuda or offsets.dtype != _I32 or offsets.dim() != 1 or offsets.numel() < 2 or \
            not offsets.is_contiguous():
        raise ValueError("sector_means: `offsets` must be a contiguous CUDA int32 [n_clouds + 1]")
    n, C = offsets.numel() - 1, feats.shape[1]
    out = torch.empty((n, 16 * C), device=feats.device, dtype=_F32)
    check(lib().lc_spconv_sector_means(feats.data_ptr(), ldf, coords.data_ptr(), offsets.data_ptr(), n, C,
                                       edges.data_ptr(), float(voxel), out.data_ptr(), _stream()),
          "lc_spconv_sector_means")
    return out


class CoordLevels:
    """The coordinate levels of one collated input (level l at stride `stride` * 2^l) and their neighbour tables, each
    built once on first use and shared by the layers over that level.  Nothing here outlives the forward that made it."""

    def __init__(self, coords: torch.Tensor, n_batch: int, max_coord: Optional[int] = None, levels: int = 5,
                 stride: int = 1):
        _req_coords(coords, "coords")
        if max_coord is None:
            max_coord = int(coords[:, :3].max().item())
        self.n_batch, self.max_coord, self.stride = int(n_batch), int(max_coord), int(stride)
        self.coords = [coords]
        for l in range(1, levels):
            self.coords.append(downsample_coords(self.coords[-1], self.stride << (l - 1)))
        self._tables, self._maps = {}, {}

    def table(self, l: int) -> torch.Tensor:
        if l not in self._tables:
            self._tables[l] = hash_build(self.coords[l], self.max_coord, self.n_batch)
        return self._tables[l]

    def _map(self, key, make):
        if key not in self._maps:
            self._maps[key] = make()
        return self._maps[key]

    def rows(self, l: int) -> int:
        return self.coords[l].shape[0]

    def same(self, l: int) -> torch.Tensor:
        return self._map(("same", l), lambda: kernel_map(self.coords[l], KIND_SAME, self.stride << l, self.table(l), self.rows(l)))

    def down(self, l: int) -> torch.Tensor:
        """[N_{l+1}, 8]: the children at level l of every voxel of level l + 1."""
        return self._map(("down", l), lambda: kernel_map(self.coords[l + 1], KIND_DOWN, self.stride << l, self.table(l),
                                                         self.rows(l)))

    def up(self, l: int) -> torch.Tensor:
        """[N_l, 8]: the parent at level l + 1 of every voxel of level l, in the slot of its offset."""
        return self._map(("up", l), lambda: kernel_map(self.coords[l], KIND_UP, self.stride << l, self.table(l + 1),
                                                       self.rows(l + 1)))
