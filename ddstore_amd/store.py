"""DDStore -- MI355X-native distributed in-HBM sample store.

Capability-parity re-design of the reference ``DDStore`` class
(reference: include/ddstore.hpp:26-258, src/ddstore.cxx:19-96) built for one
process per GPU over RCCL/xGMI:

  * each rank's shard lives in its GPU's 288 GB HBM3E (``hipMalloc`` inside
    the native :mod:`ddstore_amd._C` extension);
  * peers map each other's shards with hipIpc handles exchanged over the
    torch.distributed metadata plane (the analog of the reference's
    ``MPI_Win_create`` collective / libfabric handshake, ddstore.hpp:56-62,
    common.cxx:285-302);
  * ``get`` resolves the owning rank from the replicated prefix-sum directory
    (ddstore.hpp:75-89) and pulls peer-to-peer over xGMI -- the batched
    ``get_batch``/``get_csr`` hot path is a single hand-written CDNA4 gather
    kernel per minibatch instead of the reference's one blocking MPI_Get per
    row (ddstore.hpp:229-237);
  * ``device="cpu"`` gives the host compatibility path (BASELINE config 1):
    shards in POSIX shared memory, one-sided memcpy reads.

Unlike the reference there is exactly ONE transport per mode -- the
constructor still accepts ``method`` for API compatibility (reference
ddstore.hpp:251) but both values use the native path.
"""
from __future__ import annotations

import os
import struct
import uuid
from typing import Dict, NamedTuple, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _C
from .comm import Comm, as_comm, default_device_index

ArrayLike = Union[np.ndarray, torch.Tensor]

_ITEMSIZE_DTYPE = {1: torch.uint8, 2: torch.float16, 4: torch.float32, 8: torch.float64}

_SUPPORTED = {
    torch.uint8,
    torch.bool,
    torch.int32,
    torch.int64,
    torch.float32,
    torch.float64,
    torch.float16,
    torch.bfloat16,
    torch.float8_e4m3fn,
    torch.float8_e5m2,
}


class GraphBatch(NamedTuple):
    """One packed minibatch of graphs, as :meth:`DDStore.get_graph_batch`
    returns it (``n`` requested graphs, buffer capacities ``Ncap``/``Ecap``)."""

    x: torch.Tensor            # (Ncap, disp) packed node features
    edge_index: torch.Tensor   # (2, Ecap), or (Ecap, 2) with coo=False
    ptr: torch.Tensor          # int64 (n+1,) node offsets
    edge_ptr: torch.Tensor     # int64 (n+1,) edge offsets
    batch: torch.Tensor        # int64 (Ncap,) graph id of every node
    node_extras: tuple         # ((values, offsets), ...)
    edge_extras: tuple


class ColumnStats(NamedTuple):
    """Per-column statistics of a variable, as :meth:`DDStore.column_stats`
    returns them. Column ``c`` is flat position ``c`` of a row (CSR: of an
    element)."""

    count: int            # rows (CSR: elements) the statistics cover
    mean: torch.Tensor    # CPU float64 (disp,)
    std: torch.Tensor     # population standard deviation (divide by count)
    min: torch.Tensor
    max: torch.Tensor

    def affine(self, kind: str = "standard") -> Tuple[torch.Tensor, torch.Tensor]:
        """``(scale, shift)`` as CPU float32 vectors for the ``affine=``
        argument of the fetches, computed in float64 and rounded once.
        ``"standard"``: ``(x - mean) / std``; ``"minmax"``: ``(x - min) /
        (max - min)``. A column without spread (``std == 0`` or ``max ==
        min``) gets ``scale = 1`` and ``shift = -mean`` (``-min``): it maps to
        0, not to inf."""
        if kind == "standard":
            center, spread = self.mean, self.std
        elif kind == "minmax":
            center, spread = self.min, self.max - self.min
        else:
            raise ValueError(f"ColumnStats.affine: unknown kind '{kind}'")
        safe = torch.where(spread == 0, torch.ones_like(spread), spread)
        return (1.0 / safe).to(torch.float32), (-center / safe).to(torch.float32)


def _affine_vector(a) -> Optional[torch.Tensor]:
    """The vector form of one affine operand as a tensor, None for a number
    (Python or NumPy scalar, 0-d array or tensor)."""
    if isinstance(a, torch.Tensor):
        return a if a.dim() >= 1 else None
    if isinstance(a, (int, float, np.generic)):
        return None
    arr = np.asarray(a)
    if arr.ndim == 0:
        return None
    return torch.from_numpy(np.ascontiguousarray(arr, dtype=np.float32))


def _as_tensor(arr: ArrayLike) -> torch.Tensor:
    if isinstance(arr, torch.Tensor):
        t = arr
    elif isinstance(arr, np.ndarray):
        a = np.ascontiguousarray(arr)
        if not a.flags.writeable:
            # read-only views (e.g. io.py memmaps) are only ever READ here
            # (add/update copy into store-owned memory); silence torch's
            # non-writable warning instead of paying a host copy
            import warnings

            with warnings.catch_warnings():
                warnings.simplefilter("ignore", UserWarning)
                t = torch.from_numpy(a)
        else:
            t = torch.from_numpy(a)
    else:
        t = torch.as_tensor(arr)
    if t.dtype not in _SUPPORTED:
        raise TypeError(f"ddstore: unsupported dtype {t.dtype}")
    return t.contiguous()


class DDStore:
    """Distributed sample store: sharded rows, one-sided remote reads.

    Parameters
    ----------
    comm : None | Comm | torch.distributed group | mpi4py comm
        Metadata plane. ``None`` uses torch.distributed's WORLD if
        initialized, else a single-rank self-comm.
    method : int
        Accepted for reference API compatibility (0 = MPI RMA, 1 = libfabric
        in the reference); both values use the single native transport here.
    device : None | str | int
        ``None`` -> GPU if available else CPU; ``"cpu"`` forces the shared
        memory host path; ``"cuda"``/``"cuda:N"``/int pins a GPU.
    ddstore_width : Optional[int]
        Replication-group width (reference README.md:154-172; documented but
        NOT implemented in the reference binding, pyddstore.pyx:61 -- here it
        is a real constructor argument): ranks are split into groups of
        ``width`` consecutive ranks, each group holding a full replica
        partitioned internally.
    """

    def __init__(
        self,
        comm=None,
        method: int = 0,
        device: Union[None, str, int] = None,
        ddstore_width: Optional[int] = None,
    ):
        self.method = int(method)
        self.world_comm = as_comm(comm)
        if ddstore_width is not None and 0 < ddstore_width < self.world_comm.size:
            self.comm: Comm = self.world_comm.Split(
                self.world_comm.rank // ddstore_width, self.world_comm.rank
            )
        else:
            self.comm = self.world_comm
        self.rank = self.comm.rank
        self.size = self.comm.size

        env_dev = os.environ.get("DDSTORE_DEVICE")
        if device is None and env_dev:
            device = env_dev
        if device is None:
            device = "cuda" if torch.cuda.is_available() else "cpu"
        if isinstance(device, int):
            device = f"cuda:{device}"
        if str(device).startswith("cuda"):
            self.mode = "hip"
            d = torch.device(device)
            self.device_index = (
                d.index if d.index is not None else default_device_index()
            )
            self.device = torch.device("cuda", self.device_index)
            torch.cuda.set_device(self.device)
            self._backend = _C.DeviceStore(self.device_index, self.rank, self.size)
        else:
            self.mode = "shm"
            self.device = torch.device("cpu")
            self.device_index = -1
            session = uuid.uuid4().hex[:12]
            session = self.comm.bcast(session, root=0)
            # distinct replication groups need distinct shm namespaces
            group_id = self.world_comm.rank - self.rank
            self._backend = _C.HostStore(f"{session}g{group_id}", self.rank, self.size)
        self._vars: Dict[str, dict] = {}
        # get_graph_batch: validated (node, edge index) pairs and the cached
        # verdicts on extras, by (extra, anchor) names
        self._graph_pairs: set = set()
        self._graph_extras_ok: Dict[tuple, bool] = {}
        self._freed = False
        # per-peer traffic accounting (local vs each remote rank), enabled via
        # DDSTORE_STATS=1 -- the reference has no observability at all
        # (SURVEY §5); device-side bincount keeps the hot path async.
        self._stats_enabled = os.environ.get("DDSTORE_STATS", "0") == "1"

    # ------------------------------------------------------------------ util
    def _mkmeta(self, is_csr: bool, dtype, disp: int, counts_all) -> dict:
        meta = {
            "is_csr": is_csr,
            "dtype": dtype,
            "disp": disp,
            "nrows_total": sum(counts_all),
        }
        if self._stats_enabled:
            prefix = [0]
            for c in counts_all:
                prefix.append(prefix[-1] + int(c))
            meta["prefix_t"] = torch.tensor(prefix, dtype=torch.int64, device=self.device)
            meta["peer_rows"] = torch.zeros(self.size, dtype=torch.int64, device=self.device)
        return meta

    def _account(self, meta: dict, idx: torch.Tensor) -> None:
        if self._stats_enabled and "prefix_t" in meta:
            owner = torch.searchsorted(meta["prefix_t"], idx, right=True) - 1
            meta["peer_rows"] += torch.bincount(owner, minlength=self.size)

    def _staged(self, t: torch.Tensor) -> torch.Tensor:
        """Place an input tensor where the backend can ingest it."""
        if self.mode == "shm":
            return t.cpu()
        if t.is_cuda and t.device.index != self.device_index:
            return t.to(self.device)
        return t

    def _exchange_and_open(self, name: str) -> None:
        if self.mode == "hip":
            if self.size > 1 and getattr(self.comm, "same_process", False) is True:
                # ranks are threads of this process (the comm says so): a
                # process cannot open its own IPC handle, so the entry is
                # (pid, device pointer); the backend refuses a foreign pid
                h = struct.pack("=qQ", os.getpid(), self._backend.base_ptr(name))
            else:
                h = self._backend.ipc_handle(name) if self.size > 1 else b""
            handles = self.comm.allgather(h)
            self._backend.open_peers(name, handles)
        else:
            n = self._backend.shm_name(name)
            names = self.comm.allgather(n)
            self.comm.barrier()  # all segments exist before anyone opens
            self._backend.open_peers(name, names)
        self.comm.barrier()

    def _validate_uniform(self, disp: int, dtype: torch.dtype) -> int:
        info = self.comm.allgather((int(disp), str(dtype)))
        disps = {d for d, _ in info if d >= 0}
        if len(disps) > 1:
            raise ValueError("ddstore: disp must be uniform across ranks")  # ref ddstore.hpp:81-82
        dts = {s for _, s in info}
        if len(dts) > 1:
            raise ValueError("ddstore: dtype must be uniform across ranks")
        return disps.pop() if disps else 0

    # ------------------------------------------------------------ registration
    def add(self, name: str, arr: ArrayLike) -> None:
        """Register + ingest this rank's shard (collective; copies the data,
        the caller's array may be freed afterwards -- reference
        ddstore.hpp:39-108)."""
        t = _as_tensor(arr)
        nrows = int(t.shape[0]) if t.dim() >= 1 else 0
        disp = t.numel() // nrows if nrows > 0 else -1
        disp = self._validate_uniform(disp, t.dtype)
        nrows_all = self.comm.allgather(nrows)
        self._backend.add(name, self._staged(t), nrows, disp, nrows_all)
        self._vars[name] = self._mkmeta(False, t.dtype, disp, nrows_all)
        self._exchange_and_open(name)

    def init(
        self,
        name: str,
        nrows: int,
        disp: int,
        itemsize: int = 1,
        dtype: Optional[torch.dtype] = None,
    ) -> None:
        """Pre-allocate a zeroed shard to fill later with :meth:`update`
        (collective; reference ddstore.hpp:110-179, README.md:107)."""
        if dtype is None:
            if itemsize not in _ITEMSIZE_DTYPE:
                raise ValueError(f"ddstore init: unsupported itemsize {itemsize}")
            dtype = _ITEMSIZE_DTYPE[itemsize]
        disp = self._validate_uniform(disp, dtype)
        nrows_all = self.comm.allgather(int(nrows))
        self._backend.init(name, int(nrows), disp, torch.empty(0, dtype=dtype).dtype, nrows_all)
        self._vars[name] = self._mkmeta(False, dtype, disp, nrows_all)
        self._exchange_and_open(name)

    def update(self, name: str, arr: ArrayLike, offset: int = 0) -> None:
        """Local fill at row ``offset`` -- no communication, no epoch required
        (reference ddstore.hpp:181-195). Like the reference, separating
        updates from remote reads is the CALLER's job: write outside the
        epoch windows in which peers read (the fence choreography of
        vae-ddp.py:240-265 exists exactly for this)."""
        t = _as_tensor(arr)
        self._backend.update(name, self._staged(t), int(offset))

    def _csr_directory(self, lens: torch.Tensor):
        """Collective: allgather per-rank sample/element counts and build the
        replicated global offset directory goff[ntotal+1]."""
        nsamples = int(lens.numel())
        nelems = int(lens.sum().item()) if nsamples else 0
        nsamples_all = self.comm.allgather(nsamples)
        nelems_all = self.comm.allgather(nelems)
        lens_all = self.comm.allgather(lens.numpy())
        goff = np.zeros(sum(nsamples_all) + 1, dtype=np.int64)
        np.cumsum(np.concatenate(lens_all), out=goff[1:])
        return nsamples, nelems, nsamples_all, nelems_all, torch.from_numpy(goff)

    def _register_csr_meta(self, name: str, dtype, row_elems: int,
                           nsamples_all, goff_t: torch.Tensor) -> None:
        meta = self._mkmeta(True, dtype, row_elems, nsamples_all)
        meta["goff"] = goff_t
        if self.mode == "hip":
            meta["goff_dev"] = goff_t.to(self.device)
        self._vars[name] = meta
        self._exchange_and_open(name)

    def add_csr(self, name: str, values: ArrayLike, lengths: ArrayLike) -> None:
        """Register variable-length (CSR) samples: ``lengths[i]`` elements per
        local sample, elements of fixed feature width. First-class version of
        the reference's disp=1 element-addressed convention."""
        v = _as_tensor(values)
        lens = _as_tensor(lengths).to(torch.int64).cpu()
        nsamples, nelems, nsamples_all, nelems_all, goff_t = self._csr_directory(lens)
        row_elems = v.numel() // nelems if nelems > 0 else -1
        if nelems > 0 and v.numel() != nelems * row_elems:
            raise ValueError("ddstore add_csr: values size does not match lengths")
        row_elems = self._validate_uniform(row_elems, v.dtype)
        self._backend.add_csr(
            name, self._staged(v), nsamples, nelems, row_elems,
            nsamples_all, nelems_all, goff_t,
        )
        self._register_csr_meta(name, v.dtype, row_elems, nsamples_all, goff_t)

    def init_csr(
        self,
        name: str,
        lengths: ArrayLike,
        disp: int = 1,
        dtype: torch.dtype = torch.float32,
    ) -> None:
        """Pre-allocate a zeroed CSR variable whose per-sample LENGTHS are
        fixed now (they define the global offset directory) and whose values
        are filled later with :meth:`update_csr` -- the reference's
        incremental-fill pattern (init+update, ddstore.hpp:110-195,
        README.md:107) extended to the first-class CSR layout (collective)."""
        if dtype not in _SUPPORTED:
            raise TypeError(f"ddstore: unsupported dtype {dtype}")
        lens = _as_tensor(lengths).to(torch.int64).cpu()
        nsamples, nelems, nsamples_all, nelems_all, goff_t = self._csr_directory(lens)
        disp = self._validate_uniform(int(disp), dtype)
        st = torch.empty(0, dtype=dtype).dtype
        self._backend.init_csr(
            name, nsamples, nelems, disp, st, nsamples_all, nelems_all, goff_t
        )
        self._register_csr_meta(name, dtype, disp, nsamples_all, goff_t)

    def update_csr(self, name: str, values: ArrayLike, offset: int = 0) -> None:
        """Local fill of a CSR variable starting at local sample ``offset``:
        ``values`` holds the elements of samples ``offset, offset+1, ...``
        (any contiguous run). No communication, no epoch required -- the CSR
        analog of :meth:`update`. Like the reference, separating updates from
        remote reads is the caller's job."""
        meta = self._meta(name)
        if not meta["is_csr"]:
            raise ValueError(f"ddstore update_csr: '{name}' is not a CSR variable")
        v = _as_tensor(values)
        q = self._backend.query(name)
        p0 = int(q["prefix"][self.rank])
        ep0 = int(q["elem_prefix"][self.rank])
        nloc = int(q["nrows_local"])
        offset = int(offset)
        if not 0 <= offset <= nloc:
            raise IndexError(f"ddstore update_csr: sample offset {offset} out of range")
        elem_off = int(meta["goff"][p0 + offset].item()) - ep0
        self._backend.update_elems(name, self._staged(v), elem_off)

    # ------------------------------------------------------------------- reads
    def _check_out_dtype(self, what: str, name: str, out_dtype) -> None:
        """The store has no bool element kind (bool is stored and moved as
        bytes 0/1), so it cannot CONVERT to bool: a bool output is a byte move
        of a variable stored as bool and refused for every other variable."""
        if out_dtype == torch.bool and self._meta(name)["dtype"] != torch.bool:
            raise TypeError(
                f"ddstore {what}: bool output needs a variable stored as bool "
                f"('{name}' holds {self._vars[name]['dtype']}); fetch it as is "
                "and compare with 0")

    def _affine_operands(self, what: str, name: str, affine):
        """``(scale, shift, per_column)`` of an ``affine=`` argument: two
        floats, or -- if either operand is a vector of ``disp`` values, the
        other being broadcast -- two contiguous float32 tensors on the store
        device. A tensor that already is one is used as it is (no copy, no
        sync), so the result can be passed again at no cost."""
        disp = self._meta(name)["disp"]
        vecs = [_affine_vector(a) for a in (affine[0], affine[1])]
        if vecs[0] is None and vecs[1] is None:
            return float(affine[0]), float(affine[1]), False
        out = []
        for a, v in zip((affine[0], affine[1]), vecs):
            if v is None:
                v = torch.full((disp,), float(a), dtype=torch.float32, device=self.device)
            elif v.dim() != 1 or v.numel() != disp:
                raise ValueError(
                    f"ddstore {what}: a per-column affine operand must hold "
                    f"disp = {disp} values, got shape {tuple(v.shape)}")
            elif not (v.dtype == torch.float32 and v.device == self.device
                      and v.is_contiguous()):
                v = v.to(device=self.device, dtype=torch.float32).contiguous()
            if self.mode == "hip" and v.data_ptr() % 16:
                v = v.clone()  # the kernels load the vectors 16 B at a time
            out.append(v)
        return out[0], out[1], True

    def prepare_affine(self, name: str, affine):
        """Convert an ``affine=(scale, shift)`` argument for variable ``name``
        once: per-column operands become float32 tensors on the store device,
        which the fetches then use as they are. A scalar pair comes back as
        two floats."""
        scale, shift, _ = self._affine_operands("prepare_affine", name, affine)
        return scale, shift

    def get(self, name: str, out: ArrayLike, start: int = 0) -> None:
        """Reference-compatible dense read: fills ``out`` with rows
        ``[start, start+len(out))``; the range may not cross a shard boundary
        (reference ddstore.hpp:197-248). One-sided: only this rank
        participates."""
        if isinstance(out, np.ndarray):
            if not out.flags["C_CONTIGUOUS"]:
                raise ValueError("ddstore get: output must be C-contiguous")
            t = torch.from_numpy(out)
        elif isinstance(out, torch.Tensor):
            if not out.is_contiguous():
                raise ValueError("ddstore get: output must be C-contiguous")
            t = out
        else:
            raise TypeError("ddstore get: output must be a NumPy array or torch tensor")
        count = int(t.shape[0]) if t.dim() >= 1 else 0
        self._backend.get_range(name, int(start), count, t)

    def get_batch(
        self,
        name: str,
        indices: ArrayLike,
        out: Optional[torch.Tensor] = None,
        dtype: Optional[torch.dtype] = None,
        affine: Optional[Tuple[float, float]] = None,
    ) -> torch.Tensor:
        """The hot path: gather an arbitrary batch of global rows in one
        kernel launch (GPU: direct xGMI peer loads), packed (and optionally
        dtype-cast) into a contiguous ``(n, disp)`` tensor.

        ``affine=(scale, shift)`` fuses ``out = cast(row) * scale + shift``
        (f32 math, float output dtypes) into the gather -- data-loader
        normalization without a second pass (e.g. u8 pixels -> normalized
        bf16). Each of ``scale`` and ``shift`` is a number or a 1-D vector of
        ``disp`` values (``out[:, c] = cast(row[c]) * scale[c] + shift[c]``,
        per-feature normalization; see :meth:`column_stats`); a number beside
        a vector is broadcast, any other length raises ``ValueError``. Vectors
        that are float32 tensors on the store device are used as they are."""
        meta = self._meta(name)
        idx = torch.as_tensor(indices, dtype=torch.int64)
        idx = idx.to(self.device, non_blocking=True).contiguous()
        n = idx.numel()
        self._check_out_dtype("get_batch", name,
                              out.dtype if out is not None else dtype)
        if out is None:
            out = torch.empty(
                (n, meta["disp"]), dtype=dtype or meta["dtype"], device=self.device
            )
        self._account(meta, idx)
        if affine is not None:
            scale, shift, per_col = self._affine_operands("get_batch", name, affine)
            if out.dtype not in (torch.float32, torch.float16, torch.bfloat16):
                raise TypeError("ddstore get_batch: affine output must be float")
            if self.mode == "hip":
                if per_col:
                    self._backend.gather_affine_cols(name, idx, out, scale, shift)
                else:
                    self._backend.gather_affine(name, idx, out, scale, shift)
            else:
                tmp = torch.empty((n, meta["disp"]), dtype=meta["dtype"])
                self._backend.gather(name, idx, tmp)
                out.copy_((tmp.to(torch.float32) * scale + shift).to(out.dtype))
            return out
        if self.mode == "hip":
            self._backend.gather(name, idx, out)
        else:
            if out.dtype != meta["dtype"]:
                tmp = torch.empty((n, meta["disp"]), dtype=meta["dtype"])
                self._backend.gather(name, idx, tmp)
                out.copy_(tmp.to(out.dtype))
            else:
                self._backend.gather(name, idx, out)
        return out

    def gather_into(self, name: str, idx_dev: torch.Tensor, out: torch.Tensor) -> None:
        """Minimal-overhead gather for hot loops: ``idx_dev`` must already be a
        contiguous int64 tensor on the store device and ``out`` a matching
        output tensor (as returned/validated by a prior :meth:`get_batch`).
        Skips Python-side normalization; the native layer still validates."""
        self._check_out_dtype("gather_into", name, out.dtype)
        self._backend.gather(name, idx_dev, out)

    def get_csr(
        self,
        name: str,
        indices: ArrayLike,
        out: Optional[torch.Tensor] = None,
    ) -> Tuple[torch.Tensor, torch.Tensor]:
        """Gather variable-length samples; returns ``(values, offsets)`` where
        ``values[offsets[i]:offsets[i+1]]`` are sample ``indices[i]``'s
        elements (shape ``(total_elems, disp)``)."""
        meta = self._meta(name)
        if not meta["is_csr"]:
            raise ValueError(f"ddstore get_csr: '{name}' is not a CSR variable")
        idx = torch.as_tensor(indices, dtype=torch.int64)
        idx = idx.to(self.device, non_blocking=True).contiguous()
        if self.mode == "hip" and out is not None:
            # capacity-buffer hot path: ONE native call (lens kernel ->
            # device cumsum -> gather), no host sync, no Python between stages
            self._account(meta, idx)
            out_off = self._backend.gather_csr_fast(name, idx, out)
            return out, out_off
        out_off = torch.zeros(idx.numel() + 1, dtype=torch.int64, device=self.device)
        if self.mode == "hip":
            lens = torch.empty(idx.numel(), dtype=torch.int64, device=self.device)
            self._backend.csr_lens(name, idx, lens)
        else:
            # the host backend refuses a bad index, as its get_batch does
            if idx.numel() and not bool(((idx >= 0) & (idx < meta["nrows_total"])).all()):
                raise IndexError("ddstore get_csr: index out of range")
            goff = meta["goff"]
            lens = goff[idx + 1] - goff[idx]
        torch.cumsum(lens, 0, out=out_off[1:])
        if out is None:
            total = int(out_off[-1].item())
            out = torch.empty((total, meta["disp"]), dtype=meta["dtype"], device=self.device)
        else:
            total = out.numel() // meta["disp"]
        self._account(meta, idx)
        self._backend.gather_csr(name, idx, out_off, out, total)
        return out, out_off

    def get_csr_padded(
        self,
        name: str,
        indices: ArrayLike,
        max_len: int,
        out: Optional[torch.Tensor] = None,
        dtype: Optional[torch.dtype] = None,
        affine: Optional[Tuple[float, float]] = None,
        pad_value=0,
    ) -> Tuple[torch.Tensor, torch.Tensor]:
        """Gather variable-length samples into a fixed-shape batch; returns
        ``(dense, lengths)``.

        ``dense`` is ``(n, max_len, disp)``: ``dense[i, j]`` is element ``j``
        of sample ``indices[i]``, byte-moved, cast to ``dtype`` or run through
        ``affine=(scale, shift)`` exactly as :meth:`get_batch` does; positions
        ``j >= len_i`` hold ``pad_value`` (converted once to the output dtype,
        never cast or scaled). ``lengths`` is int64 ``(n,)`` with the TRUE
        stored length of each sample: a sample longer than ``max_len`` is
        truncated to its first ``max_len`` elements, which the caller detects
        with ``lengths > max_len`` (masks: ``lengths.clamp(max=max_len)``).
        An out-of-range index gives an all-pad row of length 0 and is counted
        in ``query()["oob_skipped"]``. On the GPU this is one kernel launch:
        no scan, no scratch, no host sync, every element written once."""
        meta = self._meta(name)
        if not meta["is_csr"]:
            raise ValueError(f"ddstore get_csr_padded: '{name}' is not a CSR variable")
        max_len = int(max_len)
        if max_len < 1:
            raise ValueError("ddstore get_csr_padded: max_len must be >= 1")
        idx = torch.as_tensor(indices, dtype=torch.int64).flatten()
        idx = idx.to(self.device, non_blocking=True).contiguous()
        n, disp = idx.numel(), meta["disp"]
        out_dtype = dtype or (out.dtype if out is not None else meta["dtype"])
        self._check_out_dtype("get_csr_padded", name, out_dtype)
        if out is not None:
            if (not out.is_contiguous() or out.device != self.device
                    or out.dtype != out_dtype or out.numel() != n * max_len * disp):
                raise ValueError(
                    "ddstore get_csr_padded: out must be a contiguous "
                    f"{out_dtype} tensor of {n}*{max_len}*{disp} elements on "
                    "the store device")
        per_col = False
        if affine is not None:
            scale, shift, per_col = self._affine_operands("get_csr_padded", name, affine)
            if out_dtype not in (torch.float32, torch.float16, torch.bfloat16):
                raise TypeError("ddstore get_csr_padded: affine output must be float")
        pad = torch.tensor([pad_value], dtype=out_dtype)  # converted once, on the host
        if n == 0:
            dense = out if out is not None else torch.empty(
                (0, max_len, disp), dtype=out_dtype, device=self.device)
            return (dense.view(0, max_len, disp),
                    torch.empty(0, dtype=torch.int64, device=self.device))
        self._account(meta, idx)
        if self.mode == "hip":
            dense = out if out is not None else torch.empty(
                (n, max_len, disp), dtype=out_dtype, device=self.device)
            lengths = torch.empty(n, dtype=torch.int64, device=self.device)
            # the pad travels as the raw bits of one output element
            bits_t = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
            pad_bits = int(pad.view(bits_t[pad.element_size()]).item())
            if per_col:
                self._backend.gather_csr_padded_cols(name, idx, dense, lengths,
                                                     max_len, pad_bits, scale, shift)
            elif affine is not None:
                self._backend.gather_csr_padded(name, idx, dense, lengths, max_len,
                                                pad_bits, True, scale, shift)
            else:
                self._backend.gather_csr_padded(name, idx, dense, lengths, max_len,
                                                pad_bits)
            return dense.view(n, max_len, disp), lengths
        # host path: ragged gather (skips and counts a bad index), then one
        # masked take into the dense layout -- each element written once
        goff = meta["goff"]
        ok = (idx >= 0) & (idx < meta["nrows_total"])
        safe = torch.where(ok, idx, torch.zeros_like(idx))
        lengths = torch.where(ok, goff[safe + 1] - goff[safe], torch.zeros_like(idx))
        off = torch.zeros(n + 1, dtype=torch.int64)
        torch.cumsum(lengths, 0, out=off[1:])
        total = int(off[-1].item())
        vals = torch.empty((total, disp), dtype=meta["dtype"])
        self._backend.gather_csr(name, idx, off, vals, total)
        pos = torch.arange(max_len, dtype=torch.int64)
        valid = pos.unsqueeze(0) < lengths.clamp(max=max_len).unsqueeze(1)
        src = (off[:-1].unsqueeze(1) + pos.unsqueeze(0)).clamp(max=max(total - 1, 0))
        if total > 0:
            x = vals[src]  # (n, max_len, disp); pad positions masked below
            if affine is not None:
                x = (x.to(torch.float32) * scale + shift).to(out_dtype)
            elif x.dtype != out_dtype:
                x = x.to(out_dtype)
            dense_v = torch.where(valid.unsqueeze(2), x, pad)
        else:
            dense_v = pad.expand(n, max_len, disp)
        if out is None:
            return dense_v.contiguous(), lengths
        out.view(n, max_len, disp).copy_(dense_v)
        return out.view(n, max_len, disp), lengths

    # ----------------------------------------------------------- graph batches
    def _graph_pair(self, node_name: str, edge_index_name: str, edge_dtype):
        """Host-side validation of a (node, edge index) pair, done once per
        pair of names; returns ``(node meta, edge meta, output dtype)``."""
        nmeta, emeta = self._meta(node_name), self._meta(edge_index_name)
        if (node_name, edge_index_name) not in self._graph_pairs:
            for nm, m in ((node_name, nmeta), (edge_index_name, emeta)):
                if not m["is_csr"]:
                    raise ValueError(
                        f"ddstore get_graph_batch: '{nm}' is not a CSR variable")
            if emeta["disp"] != 2:
                raise ValueError(
                    f"ddstore get_graph_batch: edge index '{edge_index_name}' "
                    f"must have disp == 2 (rows of (src, dst)), has {emeta['disp']}")
            if emeta["dtype"] not in (torch.int32, torch.int64):
                raise TypeError(
                    f"ddstore get_graph_batch: edge index '{edge_index_name}' "
                    f"must be int32 or int64, is {emeta['dtype']}")
            pn = list(self._backend.query(node_name)["prefix"])
            pe = list(self._backend.query(edge_index_name)["prefix"])
            if pn != pe:
                raise ValueError(
                    "ddstore get_graph_batch: node and edge variables hold "
                    "different numbers of samples per rank")
            self._graph_pairs.add((node_name, edge_index_name))
        out_dtype = edge_dtype or torch.int64
        if out_dtype not in (torch.int32, torch.int64):
            raise TypeError("ddstore get_graph_batch: edge_dtype must be int32 or int64")
        if out_dtype == torch.int32 and emeta["dtype"] != torch.int32:
            raise TypeError(
                "ddstore get_graph_batch: an int64 edge index is not narrowed to int32")
        return nmeta, emeta, out_dtype

    def _graph_extra(self, name: str, anchor: str) -> None:
        """An extra must be cut into samples exactly as its anchor variable
        (same global offsets); checked once per pair of names."""
        key = (name, anchor)
        if key not in self._graph_extras_ok:
            meta = self._meta(name)
            if not meta["is_csr"]:
                raise ValueError(f"ddstore get_graph_batch: '{name}' is not a CSR variable")
            self._graph_extras_ok[key] = torch.equal(meta["goff"],
                                                     self._meta(anchor)["goff"])
        if not self._graph_extras_ok[key]:
            raise ValueError(
                f"ddstore get_graph_batch: '{name}' does not have the sample "
                f"lengths of '{anchor}'")

    def get_graph_batch(
        self,
        node_name: str,
        edge_index_name: str,
        indices: ArrayLike,
        *,
        x_out: Optional[torch.Tensor] = None,
        edge_out: Optional[torch.Tensor] = None,
        batch_out: Optional[torch.Tensor] = None,
        coo: bool = True,
        edge_dtype: Optional[torch.dtype] = None,
        edge_fill: int = -1,
        node_extras: Sequence[str] = (),
        edge_extras: Sequence[str] = (),
    ) -> GraphBatch:
        """Fetch a minibatch of whole graphs for a message-passing model:
        packed node features, the edge index relabelled to the packed batch,
        and the batch vector. On the GPU this is one native call with no host
        sync when the three buffers are passed.

        Storage convention: graphs are the samples of two groups of CSR
        variables. Node-aligned variables (``node_name``, ``node_extras``)
        have ``lengths[i]`` = nodes of graph ``i``; edge-aligned ones
        (``edge_index_name``, ``edge_extras``) have ``lengths[i]`` = edges of
        graph ``i``. The edge index has ``disp == 2``, dtype int64 or int32:
        row ``e`` of graph ``i`` is ``(src, dst)`` with node ids LOCAL to the
        graph, in ``[0, nodes_i)`` (a ``(2, E)`` array is transposed once
        before :meth:`add_csr`). Stored ids are not validated: an id outside
        its graph gives an edge that names some other node or none.

        With ``n = len(indices)`` the result holds

        * ``x`` ``(Ncap, disp)``: exactly ``get_csr(node_name, indices,
          out=x_out)[0]``; ``ptr`` int64 ``(n+1,)`` its offsets;
        * ``edge_ptr`` int64 ``(n+1,)``: the edge offsets, never clamped;
        * ``edge_index`` ``(2, Ecap)`` (``(Ecap, 2)`` with ``coo=False``) of
          ``edge_dtype`` (default int64; int32 only for an int32 variable):
          edge ``e`` of graph ``i`` is ``stored_id + ptr[i]`` at column (row)
          ``edge_ptr[i] + e``;
        * ``batch`` int64 ``(Ncap,)``: ``batch[j] = i`` for ``ptr[i] <= j <
          ptr[i+1]``.

        ``Ncap``/``Ecap`` are the capacities of the caller's buffers: ``x_out``
        as for :meth:`get_csr`, ``batch_out`` int64 with exactly ``Ncap``
        elements, ``edge_out`` contiguous of the output dtype with exactly
        ``2 * Ecap`` elements. Pass all three or none; without them they are
        sized exactly from the host copy of the offsets (which costs a sync if
        ``indices`` lives on the device).

        Undersized buffers: graphs are kept as a prefix of the request. A
        graph's nodes are kept as :meth:`get_csr` decides (its slice ends at
        or before ``Ncap``); its edges are written only if its nodes were kept
        and its edge slice ends at or before ``Ecap``, so a written edge never
        names a node that was not written. A graph whose nodes fit but whose
        edges do not keeps its nodes, which then appear as isolated nodes; the
        caller sees it as ``edge_ptr[-1] > Ecap``, and each such graph with at
        least one edge counts once in the edge variable's ``cap_skipped``.

        Every element of ``batch`` and ``edge_index`` is written (no pre-fill
        needed): ``batch[j] = n`` for slots of no kept node -- a dummy segment,
        so a consumer can reduce into ``n + 1`` segments without a mask -- and
        ``edge_fill`` (converted once to the output dtype, never shifted) in
        every slot of no kept edge. The slack of ``x`` stays untouched. A bad
        index has length 0 in ``ptr`` and ``edge_ptr`` and counts once in
        ``oob_skipped`` of both variables.

        ``node_extras``/``edge_extras`` name further CSR variables with the
        same sample lengths as the node / edge-index variable; each is fetched
        with :meth:`get_csr` and the same indices and comes back as
        ``(values, offsets)``."""
        nmeta, emeta, out_dtype = self._graph_pair(node_name, edge_index_name,
                                                   edge_dtype)
        for nm in node_extras:
            self._graph_extra(nm, node_name)
        for nm in edge_extras:
            self._graph_extra(nm, edge_index_name)
        bufs = (x_out, edge_out, batch_out)
        if any(b is None for b in bufs) and not all(b is None for b in bufs):
            raise ValueError(
                "ddstore get_graph_batch: pass x_out, edge_out and batch_out together")
        idx = torch.as_tensor(indices, dtype=torch.int64).flatten()
        n, disp = idx.numel(), nmeta["disp"]
        fill = int(torch.tensor([edge_fill], dtype=out_dtype).item())
        if x_out is None:
            # exact sizes from the host offsets (a device `indices` syncs here)
            ih = idx.cpu()
            ih = ih[(ih >= 0) & (ih < nmeta["nrows_total"])]
            gn, ge = nmeta["goff"], emeta["goff"]
            ncap = int((gn[ih + 1] - gn[ih]).sum())
            ecap = int((ge[ih + 1] - ge[ih]).sum())
            x_out = torch.empty((ncap, disp), dtype=nmeta["dtype"], device=self.device)
            edge_out = torch.empty(2 * ecap, dtype=out_dtype, device=self.device)
            batch_out = torch.empty(ncap, dtype=torch.int64, device=self.device)
        else:
            ncap = x_out.numel() // max(disp, 1)
            if (batch_out.dtype != torch.int64 or not batch_out.is_contiguous()
                    or batch_out.device != self.device or batch_out.numel() != ncap):
                raise ValueError(
                    "ddstore get_graph_batch: batch_out must be a contiguous "
                    f"int64 tensor of {ncap} elements (x_out's capacity) on the "
                    "store device")
            if (edge_out.dtype != out_dtype or not edge_out.is_contiguous()
                    or edge_out.device != self.device or edge_out.numel() % 2):
                raise ValueError(
                    "ddstore get_graph_batch: edge_out must be a contiguous "
                    f"{out_dtype} tensor of 2 * Ecap elements on the store device")
            ecap = edge_out.numel() // 2
        if out_dtype == torch.int32 and ncap >= 2 ** 31:
            raise ValueError("ddstore get_graph_batch: int32 node ids need Ncap < 2**31")
        idx = idx.to(self.device, non_blocking=True).contiguous()
        if self.mode == "hip":
            self._account(nmeta, idx)
            self._account(emeta, idx)
            ptr, edge_ptr = self._backend.gather_graph(
                node_name, edge_index_name, idx, x_out, edge_out, batch_out,
                bool(coo), fill)
            x = x_out
        else:
            x, ptr, edge_ptr = self._graph_batch_host(
                node_name, edge_index_name, idx, x_out, edge_out, batch_out,
                ncap, ecap, bool(coo), fill)
        edge_index = edge_out.view(2, ecap) if coo else edge_out.view(ecap, 2)
        return GraphBatch(
            x, edge_index, ptr, edge_ptr, batch_out.view(ncap),
            tuple(self.get_csr(nm, idx) for nm in node_extras),
            tuple(self.get_csr(nm, idx) for nm in edge_extras))

    def _graph_batch_host(self, node_name, edge_index_name, idx, x_out, edge_out,
                          batch_out, ncap, ecap, coo, fill):
        """Host path of :meth:`get_graph_batch`: the existing CSR gather plus
        torch ops, same semantics as the kernels."""
        nmeta, emeta = self._meta(node_name), self._meta(edge_index_name)
        n = idx.numel()
        ok = (idx >= 0) & (idx < emeta["nrows_total"])
        safe = torch.where(ok, idx, torch.zeros_like(idx))

        def offsets(goff):  # a bad index has length 0
            lens = torch.where(ok, goff[safe + 1] - goff[safe], torch.zeros_like(idx))
            off = torch.zeros(n + 1, dtype=torch.int64)
            torch.cumsum(lens, 0, out=off[1:])
            return lens, off

        _, ptr = offsets(nmeta["goff"])
        elen, edge_ptr = offsets(emeta["goff"])
        # nodes: what get_csr(out=) does on this path (its gather skips and
        # counts bad indices and graphs that end past the capacity)
        self._account(nmeta, idx)
        self._backend.gather_csr(node_name, idx, ptr, x_out, ncap)
        x = x_out
        # both offset arrays are monotone: the kept graphs are prefixes
        nodes_fit = ptr[1:] <= ncap
        kn = int(nodes_fit.sum())
        ke = int((nodes_fit & (edge_ptr[1:] <= ecap)).sum())
        node_end, edge_end = int(ptr[kn]), int(edge_ptr[ke])
        batch = batch_out.view(ncap)
        batch[node_end:] = n
        batch[:node_end] = torch.repeat_interleave(
            torch.arange(kn, dtype=torch.int64), ptr[1:kn + 1] - ptr[:kn])
        # a buffer of exactly the kept edges: the gather skips and counts the
        # graphs behind it, as the relabelling kernel does
        stored = torch.empty((edge_end, 2), dtype=emeta["dtype"])
        self._backend.gather_csr(edge_index_name, idx, edge_ptr, stored, edge_end)
        shift = torch.repeat_interleave(ptr[:ke], elen[:ke]).unsqueeze(1)
        kept = (stored.to(torch.int64) + shift).to(edge_out.dtype)
        if coo:
            ev = edge_out.view(2, ecap)
            ev[:, edge_end:] = fill
            ev[:, :edge_end] = kept.t()
        else:
            ev = edge_out.view(ecap, 2)
            ev[edge_end:] = fill
            ev[:edge_end] = kept
        return x, ptr, edge_ptr

    def local_shard(self, name: str) -> torch.Tensor:
        """Zero-copy view of this rank's shard (rows x disp). Valid until
        ``free``."""
        return self._backend.local_shard(name)

    # -------------------------------------------------------------- statistics
    def _column_stats_host(self, name: str, n: int, disp: int) -> torch.Tensor:
        """Host form of the native ``column_stats``: (5, disp) float64 =
        pivot, offset (mean = pivot + offset), M2, min, max of the local
        shard. The pivot is the first row (0 where that is not finite); the
        offset is the mean of ``x - pivot`` and M2 the sum of the squares
        centred on it, so nothing is left to cancel."""
        if n == 0 or disp == 0:
            return torch.full((5, disp), float("nan"), dtype=torch.float64)
        x = self._backend.local_shard(name)
        if x.dtype.is_floating_point and x.element_size() < 4:
            x = x.to(torch.float32)  # exact, and every dtype converts from it
        x = x.to(torch.float64)
        pivot = torch.where(torch.isfinite(x[0]), x[0], torch.zeros_like(x[0]))
        d = x - pivot
        off = d.mean(0)
        m2 = ((d - off) ** 2).sum(0)
        return torch.stack([pivot, off, m2, x.amin(0), x.amax(0)])

    def column_stats(self, name: str, local: bool = False) -> ColumnStats:
        """Per-column ``(count, mean, std, min, max)`` of variable ``name``
        over all ranks of the store (collective, like :meth:`add`), or over
        this rank's shard only with ``local=True`` (not collective).

        Column ``c`` is flat position ``c`` of a row (of an element for a CSR
        variable); ``count`` is the number of rows (elements). Values are
        taken as float64 (int64 rounds to nearest), sums are accumulated in
        float64 around a per-column pivot taken from the data, so a mean that
        is large against the spread costs no accuracy; ``std`` divides by
        ``count``. ``min``/``max`` are exact. A column of equal values has
        ``std == 0.0`` exactly. A NaN anywhere in a column makes all four of
        its statistics NaN; ``count == 0`` makes everything NaN. Two calls on
        unchanged data return identical bits.

        On the GPU each rank reduces its shard with two kernels on the current
        stream (transient memory independent of the number of rows) and reads
        ``4 * disp`` numbers back with one sync; the ranks' partials are merged
        on the host. The gather counters of :meth:`query` are not touched."""
        meta = self._meta(name)
        disp = meta["disp"]
        q = self._backend.query(name)
        n = int(q["nelems_local"] if meta["is_csr"] else q["nrows_local"])
        if self.mode == "hip":
            part = self._backend.column_stats(name)
        else:
            part = self._column_stats_host(name, n, disp)
        if local or self.size == 1:
            parts = [(n, part.numpy())]
        else:
            parts = self.comm.allgather((n, part.numpy()))
        # Chan's merge of (count, mean, M2), in rank order; an empty shard
        # contributes nothing. A mean is the pair pivot + offset: the pivots
        # are values of the data, so their difference is (nearly) exact, and
        # the difference of two means does not carry the rounding of a large
        # mean into M2. The merged mean keeps the first shard's pivot.
        count = 0
        piv = off = m2 = mn = mx = torch.full((disp,), float("nan"), dtype=torch.float64)
        for k, p in parts:
            if k == 0:
                continue
            pp, po, pm2, pmn, pmx = torch.from_numpy(np.asarray(p))
            if count == 0:
                count, piv, off, m2, mn, mx = k, pp, po, pm2, pmn, pmx
                continue
            tot = count + k
            delta = (pp - piv) + (po - off)
            off = off + delta * (k / tot)
            m2 = m2 + pm2 + delta * delta * (count * k / tot)
            mn, mx = torch.minimum(mn, pmn), torch.maximum(mx, pmx)  # NaN stays
            count = tot
        mean = piv + off
        std = torch.sqrt(m2 / count) if count else m2
        flat = mn == mx  # equal values: exact, whatever the arithmetic gave
        mean = torch.where(flat, mn, mean)
        std = torch.where(flat, torch.zeros_like(std), std)
        nan = torch.isnan(mn) | torch.isnan(mx)
        nanv = torch.full_like(mean, float("nan"))
        return ColumnStats(count, *(torch.where(nan, nanv, t).clone()
                                    for t in (mean, std, mn, mx)))

    # ------------------------------------------------------------------ epochs
    def epoch_begin(self) -> None:
        """Collective epoch fence (reference MPI_Win_fence, ddstore.cxx:51-63):
        local stream fence + barrier; throws on double-begin."""
        self._backend.epoch_begin()
        self.comm.barrier()

    def epoch_end(self) -> None:
        self._backend.epoch_end()
        self.comm.barrier()

    def epoch(self):
        """Context manager form of the epoch fence:

            with store.epoch():
                batch = store.get_batch(...)
        """
        import contextlib

        @contextlib.contextmanager
        def _cm():
            self.epoch_begin()
            try:
                yield self
            finally:
                self.epoch_end()

        return _cm()

    # --------------------------------------------------------------- reshuffle
    def reshuffle(self, name: str, seed: int,
                  max_chunk_bytes: Optional[int] = None) -> None:
        """Epoch-level global data reshuffle over xGMI.

        Default: one all-to-all exchange of the whole variable
        (:func:`ddstore_amd.reshuffle.reshuffle_epoch`; transiently ~2x the
        shard). With ``max_chunk_bytes`` set: in-place cycle-order chunked
        exchange with O(chunk) transient memory -- required near HBM
        capacity (:func:`ddstore_amd.reshuffle.reshuffle_epoch_chunked`,
        fixed-stride variables only)."""
        if max_chunk_bytes is not None:
            from .reshuffle import reshuffle_epoch_chunked

            reshuffle_epoch_chunked(self, name, seed, max_chunk_bytes)
        else:
            from .reshuffle import reshuffle_epoch

            reshuffle_epoch(self, name, seed)

    # ------------------------------------------------------------ checkpoint
    def dump(self, name: str, path: str) -> None:
        """Write this rank's shard (+ metadata) to ``path`` (one file per
        rank). The reference has no checkpointing; shards there
        are rebuilt from source data every run."""
        meta = self._meta(name)
        q = self._backend.query(name)
        payload = {
            "shard": self._backend.local_shard(name).cpu().clone(),
            "disp": meta["disp"],
            "dtype": str(meta["dtype"]),
            "is_csr": meta["is_csr"],
            "rank": self.rank,
            "size": self.size,
            "prefix": list(q["prefix"]),
        }
        if meta["is_csr"]:
            payload["goff"] = meta["goff"]
            payload["elem_prefix"] = list(q["elem_prefix"])
        torch.save(payload, path)

    def load(self, name: str, path: str) -> None:
        """Collective: re-register variable ``name`` from per-rank files
        written by :meth:`dump` (same world size)."""
        payload = torch.load(path, weights_only=False)
        if payload["size"] != self.size:
            raise ValueError(
                f"ddstore load: checkpoint world size {payload['size']} != {self.size}"
            )
        if payload["rank"] != self.rank:
            raise ValueError("ddstore load: checkpoint/rank mismatch")
        shard = payload["shard"]
        if payload["is_csr"]:
            goff = payload["goff"]
            p = payload["prefix"]
            lo, hi = p[self.rank], p[self.rank + 1]
            lengths = (goff[lo + 1 : hi + 1] - goff[lo:hi]) if hi > lo else torch.zeros(
                0, dtype=torch.int64
            )
            self.add_csr(name, shard, lengths)
        else:
            self.add(name, shard)

    # ------------------------------------------------------------------- misc
    def query(self, name: str) -> dict:
        return self._backend.query(name)

    def reset_counters(self, name: str) -> None:
        """Zero a variable's skip/traffic counters (e.g. after an intentional
        out-of-range probe under ``DDSTORE_STRICT=1``)."""
        self._backend.reset_counters(name)
        meta = self._vars.get(name)
        if meta is not None and "peer_rows" in meta:
            meta["peer_rows"].zero_()

    def variables(self) -> list:
        """Names of all registered variables."""
        return list(self._vars)

    def stats(self) -> dict:
        out = {}
        for name in list(self._vars):
            q = self._backend.query(name)
            out[name] = {
                k: q[k]
                for k in (
                    "n_gather",
                    "rows_gathered",
                    "bytes_gathered",
                    "oob_skipped",
                    "cap_skipped",
                )
                if k in q
            }
            meta = self._vars[name]
            if self._stats_enabled and "peer_rows" in meta:
                pr = meta["peer_rows"].cpu().tolist()
                out[name]["rows_by_owner"] = pr
                out[name]["rows_local"] = pr[self.rank]
                out[name]["rows_remote"] = sum(pr) - pr[self.rank]
        return out

    def _meta(self, name: str) -> dict:
        if name not in self._vars:
            raise KeyError(f"ddstore: unknown variable '{name}'")
        return self._vars[name]

    def free(self) -> None:
        """Release shards, peer mappings and IPC handles (reference
        ddstore.cxx:79-96; safe to call repeatedly and at teardown)."""
        if self._freed:
            return
        try:
            self.comm.barrier()  # nobody may still be reading a peer shard
        except Exception:
            pass
        self._backend.free_all()
        self._vars.clear()
        self._freed = True

    def __reduce__(self):
        raise TypeError(
            "DDStore holds GPU/shm state and is not picklable; DataLoader "
            "workers cannot use it -- use num_workers=0 or PrefetchLoader"
        )

    def __del__(self):
        try:
            if not self._freed:
                self._backend.free_all()
        except Exception:
            pass
