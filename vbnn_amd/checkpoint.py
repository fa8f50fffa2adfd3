"""Checkpoint and resume for the fused engine (a mixin of vbnn_amd/engine.py:FusedMLP): the whole state that decides the engine's future
as host arrays (state_dict / load_state_dict), one Torch7 file of it (save / load, the `model` of main.lua:181 as data), a device digest
per tensor (vbnn_digest, csrc/digest.hip) taken before the download and checked after the upload, and the replica check of a
data-parallel all-reduce run.

STATE: per VB layer means, lvars, bias; the final Linear; Adam's t, m, v per (layer, "mean" | "var"); the draw counter; the seed; the
held pruning masks and counts. DERIVED, never stored: operand shadows, prior statistics, gradient arena, batch and predictive buffers --
prepare() and the next step rebuild them from the state. Every kernel that writes a parameter is deterministic and the noise is
counter-based Philox addressed by (seed, layer, draw, row), so an engine that loaded a state continues bit for bit like the one that
saved it.

The file is a table any Torch7 user can torch.load: format = "vbnn_amd.checkpoint", version = 1, opt, arch, engine, trainer (when a
trainer saved it). Its numbers are doubles, so what does not fit one travels as a tensor: digests and the seed as int64 tensors holding
the uint64's bits, uint32 arrays (the RandomState key) as int64. The host-side packing (pack_state / unpack_state, write_checkpoint /
read_checkpoint, rng_state_table / rng_from_table) needs no GPU.
"""
import ctypes as C
import os

import numpy as np
import torch

from . import _lib as L
from . import t7file
from . import utils as u
from .nn import Context, _ordered, _p

FORMAT, VERSION = "vbnn_amd.checkpoint", 1
_ARCH_MUST_MATCH = ("sizes", "n_classes", "criterion")        # dtype and mode may differ: the fp32 masters do not depend on them
_M64 = (1 << 64) - 1


class CheckpointError(RuntimeError):
    pass


# ---------------------------------------------------------------------------------------------- the device digest
def _digest_words(t):
    """The tensor whose 32-bit words are digested for `t`: `t` itself, or for a byte tensor whose size is no multiple of 4 a copy
    padded with zero bytes to the next word."""
    assert t.is_cuda and t.is_contiguous(), "digest: a contiguous device tensor"
    nbytes = t.numel() * t.element_size()
    if nbytes % 4:
        flat = t.reshape(-1).view(torch.uint8)
        pad = torch.zeros((nbytes + 3) // 4 * 4, dtype=torch.uint8, device=t.device)
        pad[:nbytes] = flat
        return pad, pad.numel() // 4
    return t, nbytes // 4


def digests(tensors, ctx=None):
    """vbnn_digest of every tensor in `tensors` (contiguous device tensors on one device): the launches are queued on the context's
    stream into one device array, read back with ONE synchronisation. Returns Python ints (uint64)."""
    tensors = list(tensors)
    if not tensors:
        return []
    dev = tensors[0].device
    ctx = ctx or Context.get(dev)
    out = torch.zeros(len(tensors), dtype=torch.int64, device=dev)
    keep = []
    lib = L.lib()
    for i, t in enumerate(tensors):
        w, n = _digest_words(t)
        keep.append(w)
        L.check(lib.vbnn_digest(ctx.h, _p(w) if n else None, n, 0, C.c_void_p(out.data_ptr() + 8 * i)))
    return [int(v) & _M64 for v in out.cpu().tolist()]


def digest(tensor, ctx=None):
    """The device digest of one tensor (include/vbnn_hip.h: vbnn_digest over its 32-bit words, index0 = 0) as a Python int."""
    return digests([tensor], ctx)[0]


# ---------------------------------------------------------------------------------------------- host-side packing (no GPU)
def _u64_tensor(v):
    return np.array([int(v) & _M64], dtype=np.uint64).view(np.int64)


def _u64_value(a):
    return int(np.asarray(a, dtype=np.int64).reshape(-1).view(np.uint64)[0])


def _map_leaves(obj, fn):
    if isinstance(obj, dict):
        return {k: _map_leaves(v, fn) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return [_map_leaves(v, fn) for v in obj]
    return fn(obj)


def pack_state(state):
    """An engine state as the file holds it: every digest and the seed as an int64 tensor of the uint64's bits (the file's numbers are
    doubles: exact only below 2^53). Arrays are not copied."""
    out = dict(state)
    out["seed"] = _u64_tensor(state["seed"])
    out["digests"] = _map_leaves(state["digests"], _u64_tensor)
    return out


def unpack_state(table):
    """pack_state's inverse on what t7file.load returned."""
    _check_format(table, "engine state")
    out = dict(table)
    out["seed"] = _u64_value(table["seed"])
    out["digests"] = _map_leaves(table["digests"], _u64_value)
    return out


def rng_state_table(rng):
    """np.random.RandomState's state as a table of the file's types: the 624-word key as int64, position and the two Gaussian-cache
    fields as numbers (a double holds the cached Gaussian exactly)."""
    kind, key, pos, has_gauss, cached = rng.get_state()
    assert kind == "MT19937"
    return {"key": np.asarray(key, dtype=np.uint32).astype(np.int64), "pos": int(pos), "has_gauss": int(has_gauss),
            "cached_gaussian": float(cached)}


def rng_from_table(table, rng=None):
    rng = rng or np.random.RandomState()
    rng.set_state(("MT19937", np.asarray(table["key"], dtype=np.int64).astype(np.uint32), int(table["pos"]),
                   int(table["has_gauss"]), float(table["cached_gaussian"])))
    return rng


def _check_format(table, what="checkpoint"):
    if not isinstance(table, dict) or table.get("format") != FORMAT:
        raise CheckpointError(f"not a {FORMAT} table ({what}): " +
                              (f"format = {table.get('format')!r}" if isinstance(table, dict) else type(table).__name__))
    if table.get("version") != VERSION:
        raise CheckpointError(f"{what}: format version {table.get('version')!r} is unknown here (this build reads version {VERSION})")


def write_checkpoint(path, opt, state, trainer=None):
    """ONE Torch7 file: { format, version, opt, arch, engine, trainer }, written through utils.safe_save (the previous file survives as
    `<path>.old`, utils.lua:73-80). `trainer`: { epoch, indices, rng = rng_state_table(...) } or None."""
    table = {"format": FORMAT, "version": VERSION, "arch": state["arch"], "engine": pack_state(state),
             "opt": {k: (list(v) if isinstance(v, tuple) else v) for k, v in dict(opt).items()}}
    if trainer is not None:
        table["trainer"] = {"epoch": int(trainer["epoch"]), "rng": trainer["rng"],
                            "indices": np.asarray(trainer["indices"] if trainer["indices"] is not None else [], dtype=np.int64)}
    folder, name = os.path.split(os.path.abspath(path))
    return u.safe_save(table, folder, name)


def read_checkpoint(path):
    """The table write_checkpoint wrote, the engine state unpacked; refuses anything that is not one, or another version."""
    table = t7file.load(path)
    _check_format(table, path)
    table = dict(table)
    table["engine"] = unpack_state(table["engine"])
    return table


# ---------------------------------------------------------------------------------------------- the engine's side
class _Checkpoint:
    def _refuse_sharded(self, what):
        if self.sharded:
            raise RuntimeError(f"{what}: not with the sharded update (Adam's moments and the fp32 master rows are sharded by layer rows: "
                               "gathering them into one state is the follow-up)")

    def _state_tensors(self):
        """(path, tensor) of everything state_dict downloads, in a fixed order; path = keys into the state's nested tables."""
        out = []
        for li, v in enumerate(self.vb):
            for name in ("means", "lvars", "bias"):
                out.append((("layers", li, name), getattr(v, name)))
        out += [(("weight3",), self.weight3), (("bias3",), self.bias3)]
        for li, v in enumerate(self.vb):
            for key in ("mean", "var"):
                s = self._opt_state.get((v.layer_id, key))
                if s is not None and "m" in s:
                    out += [(("adam", li, key, "m"), s["m"]), (("adam", li, key, "v"), s["v"])]
        if self._held is not None:
            out += [(("held", "masks", li), m) for li, m in enumerate(self._held)]
        return out

    @staticmethod
    def _tensor_name(path):
        return "".join(f"[{k}]" if isinstance(k, int) else (("." if i else "") + k) for i, k in enumerate(path))

    @staticmethod
    def _put(root, path, value):
        node = root
        for k in path[:-1]:
            node = node[k]
        node[path[-1]] = value

    @staticmethod
    def _get(root, path):
        node = root
        for k in path:
            node = node[k]
        return node

    def _state_skeleton(self):
        nl = len(self.vb)
        sk = {"layers": [{} for _ in range(nl)], "adam": [{} for _ in range(nl)]}
        for li, v in enumerate(self.vb):
            for key in ("mean", "var"):
                s = self._opt_state.get((v.layer_id, key))
                if s is not None and "m" in s:
                    sk["adam"][li][key] = {}
        if self._held is not None:
            sk["held"] = {"masks": [None] * nl}
        return sk

    @_ordered
    def state_dict(self):
        """The complete state that decides this engine's future, as a nested dict of host NumPy arrays and plain numbers: layers[li] =
        { means, lvars, bias }, weight3, bias3, adam[li][ "mean" | "var" ] = { t, m, v } where a slot exists, draw, seed, held = { masks
        (uint8, as they are), counts } while a mask is held, arch = { sizes, n_classes, criterion, dtype, mode }, and digests: the same
        nesting with one device digest per array, taken BEFORE the copy. Operand shadows, prior statistics, the gradient arena, batch and
        predictive buffers are derived and not part of it. Synchronises once. Refused on a sharded-update engine."""
        self._refuse_sharded("state_dict")
        self._need_gathered_parameters("state_dict")
        items = self._state_tensors()
        dev_digests = torch.zeros(max(len(items), 1), dtype=torch.int64, device=self.device)
        lib, keep, hosts = L.lib(), [], []
        for i, (_, t) in enumerate(items):
            assert t.is_contiguous()
            w, n = _digest_words(t)
            keep.append(w)
            L.check(lib.vbnn_digest(self.ctx.h, _p(w), n, 0, C.c_void_p(dev_digests.data_ptr() + 8 * i)))
        for _, t in items:                                     # behind the digests, on the same stream: pinned, so truly asynchronous
            h = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
            h.copy_(t, non_blocking=True)
            hosts.append(h)
        dig_host = torch.empty(dev_digests.shape, dtype=torch.int64, pin_memory=True)
        dig_host.copy_(dev_digests, non_blocking=True)
        torch.cuda.current_stream(self.device).synchronize()  # the ONE synchronisation
        state, dig = self._state_skeleton(), self._state_skeleton()
        for i, ((path, _), h) in enumerate(zip(items, hosts)):
            self._put(state, path, h.numpy().copy())
            self._put(dig, path, int(dig_host[i]) & _M64)
        for li, v in enumerate(self.vb):
            for key in ("mean", "var"):
                if key in state["adam"][li]:
                    state["adam"][li][key]["t"] = int(self._opt_state[(v.layer_id, key)]["t"])
        if self._held is not None:
            state["held"]["counts"] = [int(n) for n in self._held_counts]
        state.update(format=FORMAT, version=VERSION, draw=int(self.draw), seed=int(self.seed), digests=dig,
                     arch={"sizes": [int(s) for s in self.sizes], "n_classes": int(self.n_classes), "criterion": self.criterion,
                           "dtype": self.dtype, "mode": self.mode})
        return state

    @_ordered
    def load_state_dict(self, state):
        """Make this engine the one `state` (a state_dict(), or read_checkpoint(...)["engine"]) was taken from. Refused: an unknown format
        version, other layer sizes, class count or criterion; dtype and mode may differ (the fp32 master parameters and moments do not
        depend on them: an fp32-trained network can be served by a bf16 engine). Copies into the EXISTING tensors in place, so argument
        blocks and a captured step keep their addresses; allocates the Adam slots that do not exist yet and drops those the state lacks;
        sets the draw counter (the device counter of opt.device_draw by a plain fill); installs or drops the held mask; then checks every
        uploaded tensor's device digest against the recorded one and raises CheckpointError naming the tensor on a mismatch. Finally the
        derived state is rebuilt: MAP mode off, no pruned view, a new parameter version (older PruneResults are void) and prepare() -- the
        masked form when a mask came with the state. The seed comes with the state: it addresses the noise."""
        self._refuse_sharded("load_state_dict")
        _check_format(state, "load_state_dict")
        arch = state["arch"]
        mine = {"sizes": [int(s) for s in self.sizes], "n_classes": int(self.n_classes), "criterion": self.criterion}
        for k in _ARCH_MUST_MATCH:
            theirs = [int(s) for s in arch[k]] if k == "sizes" else arch[k]
            if theirs != mine[k]:
                raise CheckpointError(f"load_state_dict: the state's {k} = {theirs!r}, this engine's {mine[k]!r}")
        has_mask = isinstance(state.get("held"), dict) and bool(state["held"].get("masks"))
        if has_mask and (self.mode == "wn" or not self.fuse_kl):
            raise CheckpointError("load_state_dict: the state holds a pruning mask, which this engine cannot train under "
                                  "(hold_pruned: LRT with opt.fuse_kl only)")
        nl = len(self.vb)
        adam = state.get("adam") or [{} for _ in range(nl)]
        # ---- Adam slots: the state's set, in place where a slot exists
        for li, v in enumerate(self.vb):
            for key in ("mean", "var"):
                rec = adam[li].get(key) if isinstance(adam[li], dict) else None
                if rec is None:
                    self._opt_state.pop((v.layer_id, key), None)
                    continue
                s = self._opt_state.setdefault((v.layer_id, key), {})
                s["t"] = int(rec["t"])
                for name in ("m", "v"):
                    if name not in s or tuple(s[name].shape) != tuple(rec[name].shape):
                        s[name] = torch.zeros(rec[name].shape, dtype=torch.float32, device=self.device)
        # ---- the held mask: installed in place where one is held, allocated otherwise, or dropped
        if has_mask:
            if self._held is None:
                self._held = [torch.zeros(v.O, v.I, dtype=torch.uint8, device=self.device) for v in self.vb]
            self._held_counts = [int(n) for n in state["held"]["counts"]]
        else:
            self._held = self._held_counts = None
        # ---- every tensor, into the existing storage
        items = self._state_tensors()
        for path, t in items:
            src = np.ascontiguousarray(self._get(state, path))
            if tuple(src.shape) != tuple(t.shape) or src.dtype != np.dtype(str(t.dtype).replace("torch.", "")):
                raise CheckpointError(f"load_state_dict: {self._tensor_name(path)} is {src.dtype}{list(src.shape)} in the state, "
                                      f"{t.dtype}{list(t.shape)} in this engine")
            t.copy_(torch.from_numpy(src))
        self.seed = int(state["seed"])
        self.draw = int(state["draw"])
        if self._draw_dev is not None:
            self._draw_dev.fill_(self.draw)
        self._argcache = {}                                   # the argument blocks bake in the seed
        # ---- what arrived is what was saved: the device digests, one read-back
        got = digests([t for _, t in items], self.ctx)
        for (path, _), g in zip(items, got):
            want = int(self._get(state["digests"], path)) & _M64
            if g != want:
                raise CheckpointError(f"load_state_dict: digest mismatch in {self._tensor_name(path)}: the state records "
                                      f"{want:#018x}, the uploaded tensor gives {g:#018x} (a damaged file or transfer)")
        # ---- derived state
        self._map = False
        self._pruned = None
        self._pver += 1
        self._params_stale = False
        self.prepare()

    def save(self, path, trainer=None):
        """state_dict() as ONE file in Torch7's binary layout (vbnn_amd.t7file; write_checkpoint): { format, version, opt, arch, engine,
        trainer }. The previous file at `path` survives as `<path>.old`. Returns the path."""
        return write_checkpoint(path, self.opt, self.state_dict(), trainer)

    @classmethod
    def load(cls, path, device=None, **opt_overrides):
        """A new single-process engine built from the file's saved opt (opt_overrides: the options that should differ, e.g. dtype="bf16"
        to serve an fp32-trained network) with the file's engine state loaded and verified."""
        table = read_checkpoint(path)
        opt = dict(table["opt"])
        for name in ("exchange_mode", "exchange", "cu_budget"):                   # one process, as compact()
            opt.pop(name, None)
        opt.update(opt_overrides)
        eng = cls(opt, device=device)
        eng.load_state_dict(table["engine"])
        return eng

    @_ordered
    def check_replicas(self):
        """Data-parallel all-reduce mode: are the replicas still identical? The device digests of the parameter and Adam-moment tensors
        (8 bytes each) are all-gathered through the engine's process group; raises CheckpointError on the first tensor whose digests differ,
        naming the tensor and the ranks. A collective: every rank calls it. With world == 1 it returns at once."""
        if self.world == 1:
            return
        self._refuse_sharded("check_replicas")
        import torch.distributed as dist
        items = [(p, t) for p, t in self._state_tensors() if p[0] != "held"]
        self.finish()
        mine = torch.tensor([d - (1 << 64) if d >= (1 << 63) else d for d in digests([t for _, t in items], self.ctx)],
                            dtype=torch.int64)
        on_dev = dist.get_backend(self.pg) == "nccl"
        if on_dev:
            mine = mine.to(self.device)
        parts = [torch.empty_like(mine) for _ in range(self.world)]
        dist.all_gather(parts, mine, group=self.pg)
        table = torch.stack(parts).cpu()                                          # [rank][tensor]
        for i, (path, _) in enumerate(items):
            col = table[:, i].tolist()
            if any(c != col[0] for c in col):
                groups = {}
                for r, c in enumerate(col):
                    groups.setdefault(c & _M64, []).append(r)
                raise CheckpointError(f"check_replicas: the replicas differ in {self._tensor_name(path)}: " +
                                      "; ".join(f"ranks {rs} hold digest {d:#018x}" for d, rs in groups.items()))
