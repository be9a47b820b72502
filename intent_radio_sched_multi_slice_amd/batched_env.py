"""BatchedRanEnv: B independent RAN-slicing environments stepped by one HIP launch.

Host side of the C ABI in include/ranenv.h.  PyTorch is plumbing here (device memory,
streams); every number is produced by the gfx950 kernels in csrc/ranenv_step_body.hpp (+ ranenv_aux.hip).

gymnasium-style surface, batched (reference: ``env.reset`` / ``env.step`` simu.py:547-566):

    env = BatchedRanEnv(batch=4096, n_slices=10, n_ues=100, n_rbs=135, rbs_per_rbg=1,
                        max_ues_slice=10, n_scenarios=200)
    env.load_scenarios(tables)                     # association + slice intents
    env.bind_se_pool(se)                           # float32 [tiles, R, U] on the GPU
    env.bind_traffic_pool(bits)                    # int32   [rows, U]    on the GPU
    env.set_episodes(scenario=..., se_base=..., se_len=..., trf_base=..., trf_len=...)
    obs = env.reset()
    obs, reward, done = env.step(inter_scores, intra_choice)   # or env.step() with a device policy
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, Optional

import numpy as np
import torch

from . import _lib
from ._lib import (ACT_RELU, ACT_TANH, F_CLEAR_HISTORY_ON_RESET, F_NO_RAW_OUTPUT, F_SYNC_CHECK, INTRA_MT, INTRA_PER_SLICE, INTRA_PF,
                   INTRA_RR, NET_IN_MASK_OBS, NET_IN_OBS, NET_MAX_HIDDEN, NET_MAX_WIDTH, POLICY_EXTERNAL, POLICY_HEAD_NETWORK, POLICY_MAPF,
                   POLICY_MARR, POLICY_NETWORK, SE_GATHER, SE_STREAM, RanEnvError)
from .scenario import MAX_AGE_CAP_DEFAULT, ScenarioTables

_TORCH_DT = {"u1": torch.uint8, "i1": torch.int8, "i4": torch.int32, "i8": torch.int64, "f8": torch.float64, "f4": torch.float32}


class _DevArray:
    """Zero-copy window on handle-owned device memory (``__cuda_array_interface__``)."""

    def __init__(self, ptr: int, shape, typestr: str, owner):
        self.__cuda_array_interface__ = {
            "shape": tuple(int(x) for x in shape), "typestr": "<" + typestr if typestr not in ("i1", "u1") else "|" + typestr,
            "data": (int(ptr), False), "version": 2, "strides": None,
        }
        self._owner = owner


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else C.c_void_p(t.data_ptr())


NET_ACTIVATIONS = {"tanh": ACT_TANH, "relu": ACT_RELU}
NET_INPUTS = {"obs": NET_IN_OBS, "mask_obs": NET_IN_MASK_OBS}
HEAD_DISTS = {"gauss_clip": _lib.HEAD_DIST_GAUSS_CLIP, "gauss_tanh": _lib.HEAD_DIST_GAUSS_TANH}
HEAD_REWARDS = {"twc": 0, "colran": 1}
HEAD_SOURCES = {"head": _lib.HEAD_SRC_HEAD, "inter": _lib.HEAD_SRC_INTER}
# reward names per head policy source -> column of the recorded reward rows ("inter": the step's rows, column 0 = player_0)
HEAD_SOURCE_REWARDS = {"head": HEAD_REWARDS, "inter": {"ibsched": 0}}


def head_reward_column(observation: str, reward: Optional[str] = None) -> int:
    """The column ``collect_head`` / ``replay_sample`` select for ``reward`` under the head policy source ``observation``: "twc" /
    "colran" of the head kernel's pair under "head", "ibsched" (IBSched's player_0 reward, what IBSchedSB3 trains on) of the step's
    reward row under "inter".  None: the source's first name.  Any other combination raises ValueError."""
    if observation not in HEAD_SOURCE_REWARDS:
        raise ValueError(f"observation must be one of {sorted(HEAD_SOURCE_REWARDS)}")
    names = HEAD_SOURCE_REWARDS[observation]
    if reward is None:
        return next(iter(names.values()))
    if reward not in names:
        raise ValueError(f"reward must be one of {sorted(names)} under the head policy source {observation!r}")
    return names[reward]


def policy_net_layers(net, activation: Optional[str] = None, in_dim: Optional[int] = None, out_dim: Optional[int] = None):
    """A policy MLP as the device runs it: ``([(W [out, in], b [out]), ...], activation)`` with float32 tensors, hidden layers
    first, the output layer last.  ``net``: a ``torch.nn.Sequential`` of ``Linear`` layers with ``Tanh`` or ``ReLU`` between
    them (one kind), or a list of ``(W, b)`` pairs with ``activation`` "tanh" (default: RLlib's and SB3's) or "relu".
    Raises ValueError unless there are 1..4 hidden layers of widths 1..512, consecutive shapes chain, and the input / output
    widths equal ``in_dim`` / ``out_dim`` where given."""
    if isinstance(net, torch.nn.Module):
        if not isinstance(net, torch.nn.Sequential):
            raise ValueError("a policy net module must be a torch.nn.Sequential of Linear and Tanh / ReLU")
        layers, acts, want_linear = [], set(), True
        for m in net:
            if isinstance(m, torch.nn.Linear) and want_linear:
                b = m.bias if m.bias is not None else torch.zeros(m.out_features, device=m.weight.device)
                layers.append((m.weight.detach(), b.detach()))
            elif isinstance(m, (torch.nn.Tanh, torch.nn.ReLU)) and not want_linear:
                acts.add("tanh" if isinstance(m, torch.nn.Tanh) else "relu")
            else:
                raise ValueError(f"unexpected module {type(m).__name__}: expected Linear, activation, Linear, ..., Linear")
            want_linear = not want_linear
        if want_linear or len(acts) > 1:
            raise ValueError("a policy net ends with a Linear layer and uses one activation")
        if activation is not None and acts and activation not in acts:
            raise ValueError(f"activation {activation!r} given for a net with {acts.pop()!r}")
        activation = acts.pop() if acts else activation
    else:
        layers = [(torch.as_tensor(np.asarray(w) if not isinstance(w, torch.Tensor) else w),
                   torch.as_tensor(np.asarray(b) if not isinstance(b, torch.Tensor) else b)) for w, b in net]
    activation = "tanh" if activation is None else activation
    if activation not in NET_ACTIVATIONS:
        raise ValueError(f"unknown activation {activation!r} (tanh, relu)")
    if not 2 <= len(layers) <= NET_MAX_HIDDEN + 1:
        raise ValueError(f"{len(layers) - 1} hidden layers: 1..{NET_MAX_HIDDEN} are supported")
    out = []
    for i, (w, b) in enumerate(layers):
        if w.dim() != 2 or b.dim() != 1 or b.shape[0] != w.shape[0]:
            raise ValueError(f"layer {i}: weight {tuple(w.shape)} / bias {tuple(b.shape)} are not a Linear's [out, in] / [out]")
        if i > 0 and w.shape[1] != out[-1][0].shape[0]:
            raise ValueError(f"layer {i}: input width {w.shape[1]} after a layer of width {out[-1][0].shape[0]}")
        if i < len(layers) - 1 and not 1 <= w.shape[0] <= NET_MAX_WIDTH:
            raise ValueError(f"hidden width {w.shape[0]}: 1..{NET_MAX_WIDTH} are supported")
        out.append((w.detach().to(torch.float32).contiguous(), b.detach().to(torch.float32).contiguous()))
    if in_dim is not None and out[0][0].shape[1] != in_dim:
        raise ValueError(f"input width {out[0][0].shape[1]}, the observation has {in_dim}")
    if out_dim is not None and out[-1][0].shape[0] != out_dim:
        raise ValueError(f"output width {out[-1][0].shape[0]}, expected {out_dim}")
    return out, activation


def _depth(x) -> int:
    """Dimensions of a tensor, an array or a nested list, by its first entries"""
    if isinstance(x, (torch.Tensor, np.ndarray)):
        return x.ndim
    return 1 + _depth(x[0]) if isinstance(x, (list, tuple)) and len(x) > 0 else int(isinstance(x, (list, tuple)))


def _is_layer(x) -> bool:
    """A ``(W, b)`` pair: a 2-D weight and a 1-D bias (tensors, arrays or nested lists)"""
    return isinstance(x, (list, tuple)) and len(x) == 2 and [_depth(x[0]), _depth(x[1])] == [2, 1]


def per_slice_nets(intra):
    """``intra`` as a list of nets, one per slice index, when it is one -- a list or tuple whose entries are themselves nets: modules,
    or lists of ``(W, b)`` pairs -- else None: a single net (which may itself be a list of ``(W, b)`` pairs) or None.  Decided by
    where the ``(W, b)`` pairs sit, whatever holds the numbers: a single net's first entry is a pair, a list of nets' first entry
    is a list whose first entry is one."""
    if not isinstance(intra, (list, tuple)) or len(intra) == 0:
        return None
    first = intra[0]
    if isinstance(first, torch.nn.Module):
        return list(intra)
    if not _is_layer(first) and isinstance(first, (list, tuple)) and len(first) > 0 and _is_layer(first[0]):
        return list(intra)
    return None


def population_first(batch: int, first_env=None, sizes=None) -> np.ndarray:
    """A population's table ``first_env`` [G + 1] (member m owns envs ``first_env[m] .. first_env[m + 1] - 1``) from itself or from the
    members' ``sizes``; ValueError unless 1..64 members tile ``[0, batch)`` in order, none of them empty."""
    if (first_env is None) == (sizes is None):
        raise ValueError("give first_env or sizes")
    first = np.asarray(first_env, dtype=np.int64) if sizes is None else np.concatenate([[0], np.cumsum(np.asarray(sizes, dtype=np.int64))])
    if first.ndim != 1 or not 2 <= first.size <= _lib.POPULATION_MAX + 1:
        raise ValueError(f"a population has 1..{_lib.POPULATION_MAX} members")
    if first[0] != 0 or first[-1] != batch or np.any(np.diff(first) <= 0):
        raise ValueError(f"first_env must rise strictly from 0 to the batch, {batch}: {first.tolist()}")
    return first.astype(np.int32)


def packed_net_floats(layers, precision: str = "f32") -> int:
    """Floats of the library's packed copy of a net (ranenv_packed_net_floats: widths padded to 32, bf16 halves the weights) -- what
    decides whether ``set_population_member`` can put the net into a member of a mixed population (``population_net()["extent"]``).
    ``layers``: a net as for ``policy_net_layers``, or its widths ``[in, hidden..., out]``."""
    if precision not in _lib.NET_PRECISIONS:
        raise ValueError(f"precision must be one of {sorted(_lib.NET_PRECISIONS)}")
    dims = _net_widths(layers)
    out = C.c_int64()
    lib = _lib.load()
    _lib.check(lib, None, lib.ranenv_packed_net_floats(len(dims) - 2, (C.c_int32 * len(dims))(*dims), _lib.NET_PRECISIONS[precision], C.byref(out)),
               "ranenv_packed_net_floats")
    return out.value


def _net_widths(layers):
    """``[in, hidden..., out]`` of a net given as for ``policy_net_layers``, or as those widths themselves"""
    if isinstance(layers, (list, tuple)) and len(layers) > 0 and all(isinstance(x, (int, np.integer)) for x in layers):
        dims = [int(x) for x in layers]
    else:
        got = policy_net_layers(layers)[0]
        dims = [got[0][0].shape[1]] + [w.shape[0] for w, _ in got]
    if not 3 <= len(dims) <= NET_MAX_HIDDEN + 2:
        raise ValueError(f"{len(dims) - 2} hidden layers: 1..{NET_MAX_HIDDEN} are supported")
    return dims


def _ppo_shape_pair(actor_layers, critic_layers):
    """The two nets' shapes as ranenv_mlp (critic None: none) for the handle-free formulas"""
    mlps = []
    for layers in (actor_layers, critic_layers):
        if layers is None:
            mlps.append(None)
            continue
        dims = _net_widths(layers)
        mlp = _lib.Mlp()
        mlp.n_hidden = len(dims) - 2
        for i, d in enumerate(dims):
            mlp.dims[i] = d
        mlps.append(mlp)
    return C.byref(mlps[0]), (C.byref(mlps[1]) if mlps[1] is not None else None)


def _ppo_wide_bytes(actor_layers, critic_layers):
    actor, critic = _ppo_shape_pair(actor_layers, critic_layers)
    lds, park = C.c_int64(), C.c_int64()
    lib = _lib.load()
    _lib.check(lib, None, lib.ranenv_ppo_wide_bytes(actor, critic, C.byref(lds), C.byref(park)), "ranenv_ppo_wide_bytes")
    return lds.value, park.value


def ppo_lds_bytes(actor_layers, critic_layers=None, wide: bool = False) -> int:
    """Bytes of LDS the device PPO update needs for one member's actor / critic pair of a kind (ranenv_ppo_lds_bytes, the header's LDS
    plan; at most 163 840): what decides, before anything is bound, whether an architecture can be a member of a device-trained
    population.  ``actor_layers`` / ``critic_layers``: nets as for ``policy_net_layers``, or their widths ``[in, hidden..., out]``.
    ``wide=True``: under the wide plan of ``ppo_bind(wide=True)`` (ranenv_ppo_wide_bytes; at most 136 192 -- every net the acting
    path accepts fits it)."""
    if wide:
        return _ppo_wide_bytes(actor_layers, critic_layers)[0]
    actor, critic = _ppo_shape_pair(actor_layers, critic_layers)
    out = C.c_int64()
    lib = _lib.load()
    _lib.check(lib, None, lib.ranenv_ppo_lds_bytes(actor, critic, C.byref(out)), "ranenv_ppo_lds_bytes")
    return out.value


def sac_lds_bytes(actor_layers, critic_layers) -> int:
    """Bytes of LDS the passes of the device SAC update need for this actor / critic shape (ranenv_sac_lds_bytes, the header's LDS plan
    under "SAC update": a fixed region and the LARGER net's rows; at most 163 840), before anything is bound.  Nets as for
    ``ppo_lds_bytes``: the actor ``[10 S, hidden..., 2 S]``, one critic ``[11 S, hidden..., 1]``."""
    actor, critic = _ppo_shape_pair(actor_layers, critic_layers)
    out = C.c_int64()
    lib = _lib.load()
    _lib.check(lib, None, lib.ranenv_sac_lds_bytes(actor, critic, C.byref(out)), "ranenv_sac_lds_bytes")
    return out.value


def ppo_wide_scratch_floats(actor_layers, critic_layers=None) -> int:
    """Floats of global memory in which ONE workgroup of a wide binding parks the 32 input rows of every layer of a net -- the larger
    of the actor's and the critic's need, the two run one after the other (ranenv_ppo_wide_bytes); ``ppo_bind(wide=True)`` allocates
    members x 2 workgroups of the largest need among the bound pairs."""
    return _ppo_wide_bytes(actor_layers, critic_layers)[1]


def ppo_spread_bytes(actor_layers, critic_layers=None, slabs: int = 64, wide: bool = False) -> int:
    """Device bytes ``ppo_bind(spread=True, slabs=slabs)`` allocates for ONE kind's actor / critic pair beside the moments
    (ranenv_ppo_spread_bytes): ``slabs`` gradient slabs of the pair's packed floats and, ``wide=True``, as many shares of parked rows
    (``ppo_wide_scratch_floats``).  A handle with both kinds bound holds the sum of the two pairs'.  Nets as for ``ppo_lds_bytes``."""
    actor, critic = _ppo_shape_pair(actor_layers, critic_layers)
    out = C.c_int64()
    lib = _lib.load()
    _lib.check(lib, None, lib.ranenv_ppo_spread_bytes(actor, critic, int(slabs), 1 if wide else 0, C.byref(out)), "ranenv_ppo_spread_bytes")
    return out.value


def ppo_slices_spread_bytes(inter_actor, inter_critic, intra_actor, intra_critic, S: int, slabs: int = 64, wide: bool = False) -> int:
    """Device bytes ``ppo_bind(per_slice=True, spread=True, slabs=slabs)`` allocates beside the moments for the non-shared agent
    (ranenv_ppo_slices_spread_bytes): ``ppo_spread_bytes`` of the inter pair plus ``S`` times that of ONE slice's intra pair (every net
    as ``ppo_lds_bytes`` takes it; a critic may be None).  No handle and no device is needed: ask before binding -- at S 10, 256 slabs
    and [512] x 3 nets the answer is 12.7 gigabytes."""
    inter, intra = _ppo_shape_pair(inter_actor, inter_critic), _ppo_shape_pair(intra_actor, intra_critic)
    out = C.c_int64()
    lib = _lib.load()
    _lib.check(lib, None, lib.ranenv_ppo_slices_spread_bytes(*inter, *intra, int(S), int(slabs), 1 if wide else 0, C.byref(out)), "ranenv_ppo_slices_spread_bytes")
    return out.value


def ppo_spread_bf16_bytes(actor_layers, critic_layers=None, slabs: int = 64) -> Dict[str, int]:
    """What ``ppo_bind(spread=True, slabs=slabs, bf16=True)`` needs for ONE kind's actor / critic pair of bf16 nets, before anything is
    bound (ranenv_ppo_spread_bfloat_bytes): "lds" -- the bf16 LDS plan's bytes, which the bind refuses above 163 840 -- and "device",
    the bytes it allocates: ``slabs`` gradient slabs of the pair's float32 packed floats and per net the float32 master, Adam's m and
    v, the gradient cell and a transposed bf16 copy of the weights.  Nets as for ``ppo_lds_bytes``."""
    actor, critic = _ppo_shape_pair(actor_layers, critic_layers)
    lds, dev = C.c_int64(), C.c_int64()
    lib = _lib.load()
    _lib.check(lib, None, lib.ranenv_ppo_spread_bfloat_bytes(actor, critic, int(slabs), C.byref(lds), C.byref(dev)), "ranenv_ppo_spread_bfloat_bytes")
    return {"lds": lds.value, "device": dev.value}


def ppo_head_spread_bytes(actor_layers, critic_layers, S: int, slabs: int = 64) -> int:
    """Device bytes ``ppo_bind(head=True, spread=True, slabs=slabs)`` allocates for the head pair beside the moments
    (ranenv_ppo_head_spread_bytes): ``slabs`` gradient slabs of the pair's packed floats and ``slabs`` float64 rows of ``log_std``'s
    ``S`` partial gradients.  Nets as for ``ppo_lds_bytes``; both are required (the head update trains a pair)."""
    actor, critic = _ppo_shape_pair(actor_layers, critic_layers)
    out = C.c_int64()
    lib = _lib.load()
    _lib.check(lib, None, lib.ranenv_ppo_head_spread_bytes(actor, critic, int(S), int(slabs), C.byref(out)), "ranenv_ppo_head_spread_bytes")
    return out.value


def population_means(result: Dict[str, np.ndarray], first_env) -> Dict[str, np.ndarray]:
    """Per-member means of what ``evaluate()`` returns: every float metric [B, n_episodes, ...] -> [G, ...], the mean over the
    member's envs and episodes (``np.mean`` of the member's block); integer entries ("scenario") are left out."""
    first = np.asarray(first_env)
    return {name: np.stack([np.mean(x[lo:hi], axis=(0, 1)) for lo, hi in zip(first[:-1], first[1:])])
            for name, x in result.items() if np.issubdtype(np.asarray(x).dtype, np.floating)}


PPO_ROW_EPOCHS_CAP = 1 << 20       # rows x epochs of ONE member (one compute unit works through them); the reference's regime is 2048 x 10
# Optimiser steps of ONE member in a launch: a step zeroes the gradient, takes the norm and runs Adam over ALL parameters, a floor
# no row count lowers.  The reference's search space needs 2048 / 8 x 20 = 5120 at the most, its default regime 320; at the 0.19 ms
# ([64, 64]) .. 0.92 ms ([256, 256]) measured per 64-row step, 8192 steps are 1.6 s .. 7.5 s (an estimate; no launch of that length was measured)
PPO_STEPS_CAP = 1 << 13
# Under ppo_bind(spread=True) the rows of a minibatch are spread over the chip: no cap on rows x epochs (an int64 cannot be exceeded by
# int32 rows x int32 epochs).  The steps cap stays: a step is three launches
PPO_SPREAD_CAPS = (np.iinfo(np.int64).max, PPO_STEPS_CAP)


def ppo_hparams(G: int, epochs, minibatch, lr, clip, vf_coeff, ent_coeff, grad_clip, adv_norm, betas, eps):
    """``ranenv_ppo_hparams[G]`` of the ``ppo_update*`` methods' arguments: every one a scalar, one value for all, or a sequence of G
    values, member m's (``betas``: one pair for all; ``grad_clip`` None: 0.0, no clipping; ``adv_norm`` "minibatch", or "none" / None).
    Returns (the ctypes array, epochs int64 [G], minibatch int64 [G])."""
    def per_member(x, name, dtype=np.float64):
        a = np.asarray(x, dtype=dtype).reshape(-1) if np.ndim(x) > 0 else np.full(G, x, dtype=dtype)
        if a.size != G:
            raise ValueError(f"{name}: {a.size} values given, one per member is {G}")
        return a
    norm = [adv_norm] * G if adv_norm is None or isinstance(adv_norm, str) else list(adv_norm)
    if len(norm) != G or any(x not in ("minibatch", "none", None) for x in norm):
        raise ValueError('adv_norm is "minibatch" or None, one for all or one per member')
    cols = {"lr": per_member(lr, "lr"), "clip": per_member(clip, "clip"), "vf_coeff": per_member(vf_coeff, "vf_coeff"),
            "ent_coeff": per_member(ent_coeff, "ent_coeff"), "grad_clip": per_member(0.0 if grad_clip is None else grad_clip, "grad_clip"),
            "eps": per_member(eps, "eps"), "minibatch": per_member(minibatch, "minibatch", np.int64), "epochs": per_member(epochs, "epochs", np.int64)}
    hp = (_lib.PpoHparams * G)()
    for m in range(G):
        for k, v in cols.items():
            setattr(hp[m], k, v[m].item())
        hp[m].beta1, hp[m].beta2, hp[m].adv_norm = float(betas[0]), float(betas[1]), 1 if norm[m] == "minibatch" else 0
    return hp, cols["epochs"], cols["minibatch"]


def ppo_order_firsts(order, units: Dict[str, int], epochs, minibatch, caps=(PPO_ROW_EPOCHS_CAP, PPO_STEPS_CAP), method: str = "ppo_update",
                     per_slice: bool = False, force: bool = False) -> Dict[str, np.ndarray]:
    """The ``first_<kind>`` tables, int32 [units[kind] + 1], of an ``order`` dict as ``adapters.ppo_row_order`` returns it -- or what
    ``method`` ("ppo_update" / "ppo_update_per_slice") refuses in it: per kind "inter" / "intra" with an "order_<kind>" a contiguous
    int32 [>= max epochs, first[-1]] tensor of rows beside a table of that size (``per_slice``: which starts at 0), and no unit of
    more than ``caps[0]`` rows x epochs or ``caps[1]`` optimiser steps -- ceil(rows / minibatch) per epoch -- unless ``force``.
    ``epochs`` / ``minibatch``: per unit, or one value for all.  The units are members, or (``per_slice``) policies."""
    epochs, minibatch = (np.asarray(x, dtype=np.int64).reshape(-1) for x in (epochs, minibatch))
    max_epochs, unit = int(epochs.max()), "policy" if per_slice else "member"
    kinds = [k for k in ("inter", "intra") if order.get("order_" + k) is not None]
    if per_slice and "inter" not in kinds:
        raise ValueError("order needs order_inter / first_inter")
    firsts = {}
    for k in kinds:
        o, f, n = order["order_" + k], np.ascontiguousarray(order["first_" + k], dtype=np.int32), units[k] + 1
        if (f.size != n or (per_slice and f[0] != 0) or o.dtype != torch.int32 or o.dim() != 2 or o.shape[0] < max_epochs or o.shape[1] != int(f[-1])
                or not o.is_contiguous()):
            raise ValueError(f"order_{k}: int32 [>= {max_epochs} epochs, first_{k}[-1]] with first_{k} of {n} entries" + (" from 0" if per_slice else "")
                             + (" (adapters.ppo_row_order(..., per_slice=True))" if per_slice and k == "intra" else ""))
        rows = np.diff(f).astype(np.int64)
        if not force and int((rows * epochs).max()) > caps[0]:
            raise RanEnvError(f"{method}: a {unit} has more than {caps[0]} rows x epochs ({k}); one compute unit works "
                              f"through a {unit}'s rows -- train such a batch in torch, or pass force=True")
        steps = int((-(-rows // np.maximum(minibatch, 1)) * epochs).max())
        if not force and steps > caps[1]:
            raise RanEnvError(f"{method}: a {unit} has more than {caps[1]} optimiser steps ({k}: {steps}); every step "
                              "passes over all parameters on one compute unit -- use larger minibatches or fewer epochs, or pass force=True")
        firsts[k] = f
    if "inter" not in kinds:
        raise ValueError("order needs order_inter / first_inter")
    return firsts


class BatchedRanEnv:
    def __init__(self, batch: int, n_slices: int, n_ues: int, n_rbs: int, rbs_per_rbg: int = 1,
                 max_ues_slice: Optional[int] = None, n_scenarios: int = 1, bandwidth_hz: float = 100e6,
                 max_steps: int = 1000, hist_depth: int = 10, max_age_cap: int = MAX_AGE_CAP_DEFAULT,
                 overfulfill: float = 0.2, norm_traffic: float = 120.0, norm_ues: float = 5.0,
                 norm_se: float = 40.0, device: Optional[torch.device] = None, flags: int = 0,
                 strict_inputs: bool = False):
        """``strict_inputs``: refuse per-step inputs that are not already contiguous tensors of the right dtype on
        the env's GPU, instead of converting them (a conversion is a hidden host-to-device copy every TTI)."""
        if not torch.cuda.is_available():
            raise RanEnvError("BatchedRanEnv needs a ROCm GPU (there is no CPU fallback)")
        self.device = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")
        if self.device.type != "cuda":
            raise RanEnvError(f"device must be a GPU, got {self.device}")
        dev_index = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self.device = torch.device("cuda", dev_index)
        self.B, self.S, self.U, self.R = int(batch), int(n_slices), int(n_ues), int(n_rbs)
        self.G = int(rbs_per_rbg)
        self.Us = int(max_ues_slice if max_ues_slice is not None else max(1, n_ues // n_slices))
        self.W = 2 * self.Us + 9
        self.max_steps, self.hist_depth, self.max_age_cap = int(max_steps), int(hist_depth), int(max_age_cap)
        self.bandwidth_hz = float(bandwidth_hz)
        self.n_scenarios = int(n_scenarios)
        self.strict_inputs = bool(strict_inputs)
        self._lib = _lib.load()
        cfg = _lib.Config(_lib.ABI_VERSION, dev_index, self.B, self.S, self.U, self.R, self.G, self.Us,
                          self.hist_depth, self.max_age_cap, self.max_steps, self.n_scenarios, int(flags), 0,
                          self.bandwidth_hz, overfulfill, norm_traffic, norm_ues, norm_se)
        self._h = C.c_void_p()
        with torch.cuda.device(self.device):
            st = self._lib.ranenv_create(C.byref(cfg), C.byref(self._h))
        if st != 0:
            msg = self._lib.ranenv_last_error(None)
            raise RanEnvError(f"ranenv_create failed ({st}): {msg.decode() if msg else ''}")
        self._keep: Dict[str, object] = {}
        self._views: Optional[Dict[str, torch.Tensor]] = None
        B, S = self.B, self.S
        dev = self.device
        self.obs_inter = torch.zeros((B, S * 10), dtype=torch.float32, device=dev)
        self.obs_intra = torch.zeros((B, S, self.W), dtype=torch.float32, device=dev)
        self.reward = torch.zeros((B, S + 1), dtype=torch.float64, device=dev)
        self.done = torch.zeros((B,), dtype=torch.uint8, device=dev)
        self.tables: Optional[ScenarioTables] = None
        self.episodes: Optional[np.ndarray] = None
        # cached ctypes views of the output buffers (the per-step call is on the hot path)
        self._obs_dict = {"obs_inter": self.obs_inter, "obs_intra": self.obs_intra}
        self._p_out = (_ptr(self.obs_inter), _ptr(self.obs_intra), _ptr(self.reward), _ptr(self.done))
        self._step_fn = self._lib.ranenv_step
        self.policy, self.fixed_intra = POLICY_MARR, INTRA_RR      # the library's defaults (ranenv_create)
        self.traffic_seed, self.env_id_base = None, 0
        self._recorder = self._trace = None      # record() / bind_trace(): a handle holds one trace, the recorder's or the caller's
        self._autoreset = False
        self.term_obs_inter = self.term_obs_intra = self.term_head_obs = None
        self.se_mode = "stream"
        self._ranges = None          # set_ranges(): [(lo, hi)] for step_async / step_wait
        self._intra_layout = None    # input layout of the intra actor bound by set_policy_network (None: none)
        self._population = None      # set_population's first_env table [G + 1] (None: no grouping)
        self._gae_per_member = False # collect() has set the members' (gamma, lambda) pairs (ranenv_set_population_gae)
        self.head_observation = "head"      # what the head nets read (set_head_policy_network): "head" = head_obs, "inter" = obs_inter
        # (the views are handed out once, here: ranenv_get_views ends the library's host shadow of the step counters -- the views are writable --,
        # and a first views() call in the middle of an auto-reset loop would switch the shortcut of enable_autoreset off until the next full reset)
        self.views()

    # ------------------------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self._lib.ranenv_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, status: int, what: str):
        _lib.check(self._lib, self._h, status, what)

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _dev(self, x, dtype, shape, name):
        if x is None:
            return None
        if self.strict_inputs and not (isinstance(x, torch.Tensor) and x.device == self.device and x.dtype == dtype
                                       and x.is_contiguous()):
            raise RanEnvError(f"{name}: strict_inputs needs a contiguous {dtype} tensor on {self.device}")
        t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.array(x, copy=True))
        t = t.to(device=self.device, dtype=dtype).contiguous()
        if tuple(t.shape) != tuple(shape):
            raise RanEnvError(f"{name}: expected shape {tuple(shape)}, got {tuple(t.shape)}")
        return t

    # ------------------------------------------------------------------------------------------
    def load_scenarios(self, tables: ScenarioTables, first: int = 0):
        """Association + slice intents (associations/mult_slice.py:350-488) into the pool."""
        if (tables.n_slices, tables.n_ues, tables.max_ues_slice) != (self.S, self.U, self.Us):
            raise RanEnvError("scenario tables do not match the env sizes")
        tables.validate(self.max_age_cap, self.R, self.bandwidth_hz)
        ct = _lib.ScenarioTablesC()
        keep = []
        for name in _lib.SCENARIO_FIELDS:
            dt = np.float64 if name in _lib.SCENARIO_F64 else np.int32
            a = np.ascontiguousarray(getattr(tables, name), dtype=dt)
            keep.append(a)
            setattr(ct, name, a.ctypes.data)
        with torch.cuda.device(self.device):
            self._check(self._lib.ranenv_load_scenarios(self._h, int(first), tables.n_scenarios, C.byref(ct),
                                                         self._stream()), "ranenv_load_scenarios")
        if first == 0 and tables.n_scenarios == self.n_scenarios:
            self.tables = tables

    def bind_se_pool(self, se_pool: torch.Tensor, layout: Optional[str] = None, keep_rb_major: bool = False):
        """float32 [n_tiles, R, U] (RB-major tiles, the order of the reference's .mat: channels/quadriga.py:70-72) resident on
        this GPU.  ``layout``: how the library replays it -- ``"quad"`` (default; ``RANENV_SE_LAYOUT`` overrides): a COPY in
        RB-quad-major order [n_tiles, ceil(R/4), U, 4] is made once (ranenv_se_retile_quad, the same size again) and bound
        (ranenv_bind_se_pool_quad): 16-byte loads, a quarter of the memory instructions, bit-identical results.  The handle
        then does NOT alias the caller's tensor: writes to ``se_pool`` after this call are not seen (bind again), and this
        object keeps no reference to the RB-major tensor -- the caller may drop it and halve the pool's footprint -- unless
        ``keep_rb_major`` (then it is kept in ``self.se_pool_rb_major``).  ``"rb"``: the tensor itself is bound, zero-copy
        (ranenv_bind_se_pool).  A 4-D [n_tiles, ceil(R/4), U, 4] tensor is taken as already re-tiled (zero-copy)."""
        if se_pool.dtype != torch.float32 or se_pool.device != self.device or not se_pool.is_contiguous():
            raise RanEnvError("SE pool must be a contiguous float32 tensor on the env's GPU")
        Rq = (self.R + 3) // 4
        if se_pool.dim() == 4:
            if tuple(se_pool.shape[1:]) != (Rq, self.U, 4):
                raise RanEnvError(f"RB-quad-major SE pool must be [tiles, {Rq}, U={self.U}, 4], got {tuple(se_pool.shape)}")
            quad = se_pool
        else:
            if se_pool.dim() != 3 or se_pool.shape[1] != self.R or se_pool.shape[2] != self.U:
                raise RanEnvError(f"SE pool must be [tiles, R={self.R}, U={self.U}], got {tuple(se_pool.shape)}")
            layout = layout or os.environ.get("RANENV_SE_LAYOUT") or "quad"
            if layout not in ("quad", "rb"):
                raise RanEnvError("layout must be 'quad' or 'rb'")
            quad = None
            if layout == "quad":
                quad = torch.empty((se_pool.shape[0], Rq, self.U, 4), dtype=torch.float32, device=self.device)
                with torch.cuda.device(self.device):
                    st = self._lib.ranenv_se_retile_quad(_ptr(se_pool), _ptr(quad), se_pool.shape[0], self.U, self.R, self._stream())
                if st != 0:
                    raise RanEnvError("ranenv_se_retile_quad failed: " + (self._lib.ranenv_last_error(None) or b"").decode())
                # the copy is read by launches on other streams (partitions, ranges): a one-off build ends with a synchronisation, like
                # the gather sidecars', instead of an event every such stream would have to wait for
                torch.cuda.current_stream(self.device).synchronize()
        self.se_pool_rb_major = se_pool if (keep_rb_major and se_pool.dim() == 3) else None
        if quad is not None:
            self._keep["se_pool"] = quad
            self._check(self._lib.ranenv_bind_se_pool_quad(self._h, _ptr(quad), quad.shape[0], Rq * self.U * 4), "ranenv_bind_se_pool_quad")
            self.se_layout = "quad"
        else:
            self._keep["se_pool"] = se_pool
            self._check(self._lib.ranenv_bind_se_pool(self._h, _ptr(se_pool), se_pool.shape[0], self.R * self.U),
                        "ranenv_bind_se_pool")
            self.se_layout = "rb"
        self.se_mode = "stream"
        if os.environ.get("RANENV_SE_MODE") == "gather":       # experiment / test knob, like RANENV_SMALL_BATCH
            self.set_se_mode("gather")

    @property
    def bound_se_pool(self) -> Optional[torch.Tensor]:
        """The SE pool tensor the handle replays (RB-quad-major 4-D, or the caller's RB-major 3-D tensor under layout "rb")."""
        return self._keep.get("se_pool")

    def pooled_tiles(self, tile_index: torch.Tensor) -> torch.Tensor:
        """Tiles of the bound pool as float32 [n, R, U] (RB-major, the reference's order) whatever layout is bound."""
        pool = self._keep["se_pool"]
        t = pool.index_select(0, tile_index.to(torch.int64))
        if t.dim() == 4:                              # RB-quad-major [n, Rq, U, 4] -> [n, 4 Rq, U] -> the first R RBs
            t = t.permute(0, 1, 3, 2).reshape(t.shape[0], -1, self.U)[:, :self.R, :]
        return t

    def set_se_mode(self, mode: str):
        """``"stream"`` (default): every TTI streams the env's whole U x R tile.  ``"gather"``: the per-UE mean over all
        RBs -- all that the observation, PF / MT and MAPF read of a tile (agents/ib_sched.py:110-116,146-157,
        agents/common.py:567-573,648-654), a function of the tile alone -- is computed once per pooled tile, and a TTI reads
        that row plus, from a UE-major copy of the pool, only the RBs each UE was allocated.  Bit-identical results; the two
        sidecars (n_tiles * U * (8 + 4 * roundup(R, 8)) bytes) are built here for the pool bound now."""
        if mode not in ("stream", "gather"):
            raise RanEnvError("SE mode must be 'stream' or 'gather'")
        with torch.cuda.device(self.device):
            self._check(self._lib.ranenv_set_se_mode(self._h, SE_GATHER if mode == "gather" else SE_STREAM, self._stream()),
                        "ranenv_set_se_mode")
        self.se_mode = mode

    def bind_se_gather_from_power(self, power: torch.Tensor, transmission_power: float = 100.0,
                                  thermal_noise_power: float = 10e-14):
        """Gather-only channel ingest (channels/quadriga.py:56-76): QuaDRiGa received power, float64 [n_tiles, R, U] on this GPU
        (the .mat's own RB-major order), straight into the gather mode's sidecars -- no RB-major float32 pool is built or kept.
        Same sidecars bit for bit as ``bind_se_pool(quadriga_pool_from_power(power, R))`` + ``set_se_mode("gather")``."""
        if power.dtype != torch.float64 or power.device != self.device or power.dim() != 3 or tuple(power.shape[1:]) != (self.R, self.U):
            raise RanEnvError(f"power must be a float64 [n_tiles, R={self.R}, U={self.U}] tensor on {self.device}")
        power = power.contiguous()
        with torch.cuda.device(self.device):
            self._check(self._lib.ranenv_bind_se_gather_from_power(self._h, _ptr(power), power.shape[0],
                                                                  float(transmission_power) / float(self.R),
                                                                  float(thermal_noise_power), self._stream()),
                        "ranenv_bind_se_gather_from_power")
        self._keep.pop("se_pool", None)
        self._n_se_tiles = int(power.shape[0])
        self.se_mode = "gather"

    def se_sidecars(self) -> Dict[str, torch.Tensor]:
        """Diagnostic: the gather mode's sidecars, zero copy: ``row_mean`` float64 [tiles, U], ``ue_major`` float32
        [tiles, U, roundup(R, 8)]."""
        mean, um, rp = C.c_void_p(), C.c_void_p(), C.c_int32()
        self._check(self._lib.ranenv_get_se_sidecars(self._h, C.byref(mean), C.byref(um), C.byref(rp)), "ranenv_get_se_sidecars")
        n = self._keep["se_pool"].shape[0] if "se_pool" in self._keep else self._n_se_tiles
        return {"row_mean": torch.as_tensor(_DevArray(mean.value, (n, self.U), "f8", self), device=self.device),
                "ue_major": torch.as_tensor(_DevArray(um.value, (n, self.U, rp.value), "f4", self), device=self.device)}

    # ------------------------------------------------------------------------------------------
    # scenario load: the agent-independent figures of results/gen_results.py, without a single env step
    def se_tile_stats(self, rebuild: bool = False) -> torch.Tensor:
        """Per-tile statistics of the bound SE pool, zero copy: float64 [n_tiles, 4, U] = np.mean, np.std (population), np.min,
        np.max of every UE's SE over the R RBs, bit for bit numpy's on the float64 of the float32 values.  Built on first use for
        the pool bound now (one streaming pass; ``rebuild``: again, after the pool's contents changed); binding another pool
        drops them.  The reference's ``ues_spectral_efficiencies`` (gen_results.py:260-276) at TTI t of an episode is row
        ``se_base + (se_offset + t) % se_len``."""
        stats, n = C.c_void_p(), C.c_int64()
        with torch.cuda.device(self.device):
            if rebuild or self._lib.ranenv_get_se_stats(self._h, C.byref(stats), C.byref(n)) != 0:
                self._check(self._lib.ranenv_build_se_stats(self._h, self._stream()), "ranenv_build_se_stats")
            self._check(self._lib.ranenv_get_se_stats(self._h, C.byref(stats), C.byref(n)), "ranenv_get_se_stats")
        return torch.as_tensor(_DevArray(stats.value, (int(n.value), 4, self.U), "f8", self), device=self.device)

    def scenario_load(self, episodes=None, n_steps: Optional[int] = None, per_step: bool = False) -> Dict[str, torch.Tensor]:
        """How many RBs the network would need to serve every slice's requested traffic (gen_results.py:361-497, :1251-1451), per
        episode descriptor, from the tile statistics and the scenario rows alone.  ``episodes``: a structured array as
        ``set_episode_table`` / ``episode_descriptors`` keep them (default: the bound episode table, else the envs' current
        descriptors); ``n_steps``: TTIs per episode (default ``max_steps``).  -> ``episode_mean`` float64 [n, 3]: the mean over the
        steps of the network's (avg, min, max) needed RBs -- column 0 is what the reference ranks scenarios by
        (``scenario.rank_by_load``), and more than R there means no agent can meet that episode's intents on average.  With
        ``per_step`` also ``per_step_network`` [n, T, 3] and ``per_step_slice`` [n, T, S, 6] (avg / min / max needed RBs, then the
        capacity per RB in Mbps from the mean / min / max SE; the columns are spelled out in include/ranenv.h)."""
        if episodes is None:
            episodes = getattr(self, "episode_table", None)
            if episodes is None:
                episodes = self.episode_descriptors()
        if episodes is None:
            raise RanEnvError("scenario_load: no episodes given and none set (set_episode_table / set_episodes)")
        eps = np.ascontiguousarray(np.atleast_1d(episodes), dtype=self._EP_DTYPE)
        n, T = int(eps.shape[0]), int(self.max_steps if n_steps is None else n_steps)
        self.se_tile_stats()
        out = {"episode_mean": torch.empty((n, 3), dtype=torch.float64, device=self.device)}
        if per_step:
            out["per_step_slice"] = torch.empty((n, max(T, 0), self.S, _lib.LOAD_SLICE_COLS), dtype=torch.float64, device=self.device)
            out["per_step_network"] = torch.empty((n, max(T, 0), 3), dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            self._check(self._lib.ranenv_rbs_needed(self._h, C.c_void_p(eps.ctypes.data), n, T, _ptr(out.get("per_step_slice")),
                                                    _ptr(out.get("per_step_network")), _ptr(out["episode_mean"]), self._stream()),
                        "ranenv_rbs_needed")
        return out

    def bind_traffic_pool(self, traffic_pool: torch.Tensor):
        """int32 [rows, U] offered bits per UE and TTI (traffics/mult_slice.py:26-32)."""
        if traffic_pool.dtype != torch.int32 or traffic_pool.device != self.device or not traffic_pool.is_contiguous():
            raise RanEnvError("traffic pool must be a contiguous int32 tensor on the env's GPU")
        if traffic_pool.dim() != 2 or traffic_pool.shape[1] != self.U:
            raise RanEnvError(f"traffic pool must be [rows, U={self.U}]")
        self._keep["trf_pool"] = traffic_pool
        self._check(self._lib.ranenv_bind_traffic_pool(self._h, _ptr(traffic_pool), traffic_pool.shape[0]),
                    "ranenv_bind_traffic_pool")

    def set_episodes(self, scenario, se_base=0, se_len=1, se_offset=0, trf_base=0, trf_len=1, trf_offset=0):
        """Which scenario / channel trace / traffic trace each env replays (arrays of [B] or scalars)."""
        eps = self._episode_array(self.B, scenario, se_base, se_len, se_offset, trf_base, trf_len, trf_offset)
        with torch.cuda.device(self.device):
            self._check(self._lib.ranenv_set_episodes(self._h, C.c_void_p(eps.ctypes.data), self._stream()),
                        "ranenv_set_episodes")
        self.episodes = eps

    def set_policy(self, policy: int = POLICY_EXTERNAL, fixed_intra: int = INTRA_PER_SLICE):
        self._check(self._lib.ranenv_set_policy(self._h, int(policy), int(fixed_intra)), "ranenv_set_policy")
        self.policy, self.fixed_intra = int(policy), int(fixed_intra)

    def net_input_dims(self, intra_input: str = "obs"):
        """Input widths of the policy nets: (inter, intra) for the intra input layout "obs" or "mask_obs"."""
        if intra_input not in NET_INPUTS:
            raise ValueError(f"intra_input must be one of {sorted(NET_INPUTS)}")
        return 10 * self.S, self.W + (self.Us if intra_input == "mask_obs" else 0)

    def set_policy_network(self, inter, intra=None, stochastic: bool = False, seed: int = 0, intra_input: str = "obs",
                           activation: Optional[str] = None, fixed_intra: Optional[int] = None, precision: str = "f32", mixed: bool = False):
        """Run trained IBSched policy nets on the device in front of every TTI (RANENV_POLICY_NETWORK, include/ranenv.h):
        ``inter`` -> 2*S outputs (mean, log_std of the masked Gaussian), ``intra`` (None = ``fixed_intra``) -> 3 logits per
        (env, slice) from ``obs_intra`` ("obs") or ``[mask_intra, obs_intra]`` ("mask_obs", RLlib's flattened Dict).  Nets as
        for ``policy_net_layers``.  Switches the policy to NETWORK: ``step()`` / ``rollout()`` / ``evaluate()`` then need no
        actions.  ``stochastic``: sample (Philox noise keyed by ``seed``) instead of taking the mode.
        ``intra`` may be a list of S nets of one shape, non-shared intra policies (the reference's ``shared_policies=False``):
        ``intra[s]`` serves slice index s, i.e. ``player_{s+1}`` (ranenv_set_intra_policy_networks).
        ``precision`` "bf16": every net of this call runs on the bf16 matrix cores -- weights rounded once at bind, input and hidden
        activations rounded to bf16, float32 accumulation, biases, activations and outputs (the contract is in include/ranenv.h;
        ``adapters._mlp_forward(..., precision="bf16")`` restates it).  Results then differ from the float32 nets' in the third or
        fourth digit; "f32", the default, leaves them as they were.
        ``inter`` may be a list of G nets of one shape under ``set_population`` -- member m's envs act on ``inter[m]`` -- and ``intra``
        then None or a list of G nets (ranenv_set_population_policy); a list of S intra nets beside ONE inter net keeps its per-slice
        meaning.  ``mixed=True`` (lists under ``set_population`` only): the members' nets may differ in hidden widths, depth and
        activation -- the trials of a hyper-parameter search -- (ranenv_set_population_policy_mixed); input and output width, layout and
        precision stay common and are checked per net before any library call."""
        in_inter, in_intra = self.net_input_dims(intra_input)
        members = per_slice_nets(inter)
        if mixed and members is None:
            raise ValueError("mixed=True takes a list of inter nets, one per member of the population")
        if members is not None:                # a population: inter[m] (and intra[m]) are member m's
            G = self._population_size(len(members))
            lists = [self._net_list(members, activation, in_inter, 2 * self.S, NET_IN_OBS, precision, count=G, per="member", mixed=mixed),
                     self._member_list(intra, G, activation, in_intra, 3, NET_INPUTS[intra_input], precision, mixed)]
            self._set_population_nets("ranenv_set_population_policy" + ("_mixed" if mixed else ""), "population_policy", G, lists, 1 if stochastic else 0,
                                      int(seed) & (2 ** 64 - 1))
            for key in ("policy_net", "intra_policy_nets"):
                self._keep.pop(key, None)
            self._intra_layout = None if intra is None else NET_INPUTS[intra_input]
            self._policy_views = None
            self.set_policy(POLICY_NETWORK, self.fixed_intra if fixed_intra is None else fixed_intra)
            return
        per_slice = self._net_list(per_slice_nets(intra), activation, in_intra, 3, NET_INPUTS[intra_input], precision)
        self._set_nets("policy_net", "ranenv_set_policy_network", [(inter, activation, in_inter, 2 * self.S, NET_IN_OBS),
                       (None if per_slice else intra, activation, in_intra, 3, NET_INPUTS[intra_input])], 1 if stochastic else 0,
                       int(seed) & (2 ** 64 - 1), precision=precision)
        self._set_net_list("intra_policy_nets", "ranenv_set_intra_policy_networks", per_slice)
        self._intra_layout = None if intra is None else NET_INPUTS[intra_input]
        self._policy_views = None
        self.set_policy(POLICY_NETWORK, self.fixed_intra if fixed_intra is None else fixed_intra)

    def _mlp_struct(self, layers, act: str, layout: int, keep: list, precision="f32"):
        """``precision``: a name of ``_lib.NET_PRECISIONS`` (or, for the library's own check, the raw integer of the field)."""
        if not isinstance(precision, int) and precision not in _lib.NET_PRECISIONS:
            raise ValueError(f"precision must be one of {sorted(_lib.NET_PRECISIONS)}")
        m = _lib.Mlp()
        m.n_hidden, m.activation, m.input_layout = len(layers) - 1, NET_ACTIVATIONS[act], layout
        m.precision = precision if isinstance(precision, int) else _lib.NET_PRECISIONS[precision]
        m.dims[0] = layers[0][0].shape[1]
        for i, (w, b) in enumerate(layers):
            w, b = w.to(self.device).contiguous(), b.to(self.device).contiguous()
            keep += [w, b]
            m.dims[i + 1] = w.shape[0]
            m.weight[i], m.bias[i] = w.data_ptr(), b.data_ptr()
        return m

    def _set_nets(self, key: str, call: str, nets, *args, keep=(), precision="f32"):
        """One ``ranenv_set_*`` call that binds nets: per ranenv_mlp argument ``(net, activation, in_dim, out_dim, input layout)`` --
        a ``None`` net is passed as NULL, a callable layout is asked with the net's layers -- then ``args``, then the stream."""
        keep, structs = list(keep), []
        for net, activation, in_dim, out_dim, layout in nets:
            if net is None:
                structs.append(None)
                continue
            layers, act = policy_net_layers(net, activation, in_dim, out_dim)
            structs.append(C.byref(self._mlp_struct(layers, act, layout(layers) if callable(layout) else layout, keep, precision)))
        with torch.cuda.device(self.device):
            self._check(getattr(self._lib, call)(self._h, *structs, *args, self._stream()), call)
        self._keep[key] = keep                 # (the library copies on the current stream; keep the sources until it has)

    def _net_list(self, nets, activation, in_dim, out_dim, layout, precision="f32", count=None, per="slice", mixed=False):
        """A list of S nets as the argument of a ``ranenv_set_intra_*_networks`` call: ``(array of ranenv_mlp pointers, what to
        keep alive)``, or None for None.  Raises ValueError -- before any library call: a per-slice bind is two of
        them, and the first one drops the previous set -- unless there are S valid nets of one shape and activation.
        ``count`` / ``per``: a population's list instead, one net per member; ``mixed``: its nets may differ in hidden shape and
        activation, and must still agree in input layout."""
        if nets is None:
            return None
        if per == "member" and len(nets) != count:
            raise ValueError(f"{len(nets)} nets given: one per member is {count}")
        if per == "slice" and len(nets) != self.S:
            raise ValueError(f"{len(nets)} intra nets given: one per slice is {self.S}")
        keep, structs, first = [], [], None
        for i, net in enumerate(nets):
            layers, act = policy_net_layers(net, activation, in_dim, out_dim)
            shape = ([tuple(w.shape) for w, _ in layers], act)
            first = shape if first is None else first
            if mixed:
                if structs and (layout(layers) if callable(layout) else layout) != structs[0].input_layout:
                    raise ValueError(f"net {i} reads another input layout than net 0: the nets per member have one input layout")
            elif shape != first:
                raise ValueError(f"{'intra ' if per == 'slice' else ''}net {i} ({shape[0]}, {shape[1]}) differs from net 0 ({first[0]}, {first[1]}): "
                                 f"the nets per {per} have one shape and one activation")
            structs.append(self._mlp_struct(layers, act, layout(layers) if callable(layout) else layout, keep, precision))
        return (C.POINTER(_lib.Mlp) * len(structs))(*[C.pointer(m) for m in structs]), keep + structs

    def _set_net_list(self, key: str, call: str, net_list):
        self._keep.pop(key, None)              # (the call in front of this one has unbound the set)
        if net_list is None:
            return
        with torch.cuda.device(self.device):
            self._check(getattr(self._lib, call)(self._h, self.S, net_list[0], self._stream()), call)
        self._keep[key] = net_list[1]

    # ---- populations (ranenv_set_population ...; include/ranenv.h "Populations") ----------------------------------------------------
    def set_population(self, first_env=None, sizes=None) -> None:
        """Group the batch into G <= 64 members of contiguous envs: member m owns ``first_env[m] .. first_env[m + 1] - 1``
        (``first_env`` [G + 1], from 0 to B), or give the members' ``sizes``.  ``set_policy_network`` / ``set_value_network`` then take
        lists of G nets, and every policy launch acts on an env with its member's weights.  Neither argument: remove the grouping
        (and the population's nets).  The grouping cannot change while population nets are bound."""
        if first_env is None and sizes is None:
            self._check(self._lib.ranenv_set_population(self._h, 0, None), "ranenv_set_population")
            self._population = None
            self._gae_per_member = False     # (the library drops the members' GAE pairs with the grouping)
            for key in ("population_policy", "population_value"):
                self._keep.pop(key, None)
            return
        first = population_first(self.B, first_env, sizes)
        self._check(self._lib.ranenv_set_population(self._h, len(first) - 1, first.ctypes.data_as(C.POINTER(C.c_int32))), "ranenv_set_population")
        self._population = first

    def population(self) -> Optional[np.ndarray]:
        """The grouping as the library holds it: ``first_env`` [G + 1], or None."""
        n, first = C.c_int32(), (C.c_int32 * (_lib.POPULATION_MAX + 1))()
        self._check(self._lib.ranenv_get_population(self._h, C.byref(n), first), "ranenv_get_population")
        return np.array(first[:n.value + 1], dtype=np.int32) if n.value > 0 else None

    def population_slices(self):
        """The G Python slices of the members' envs: ``rec[k][:, sl]`` of a ``collect()`` record, ``x[sl]`` of a [B, ...] tensor --
        views, members being contiguous."""
        first = self._population_first()
        return [slice(int(lo), int(hi)) for lo, hi in zip(first[:-1], first[1:])]

    def _population_first(self) -> np.ndarray:
        if getattr(self, "_population", None) is None:
            raise ValueError("no population set (set_population)")
        return self._population

    def _population_size(self, n_given: int) -> int:
        G = len(self._population_first()) - 1
        if n_given != G:
            raise ValueError(f"{n_given} nets given: one per member is {G}")
        return G

    def _member_list(self, nets, G, activation, in_dim, out_dim, layout, precision, mixed=False):
        """The intra argument beside a list of G inter nets: None, or a list of G nets"""
        if nets is None:
            return None
        as_list = per_slice_nets(nets)
        if as_list is None:
            raise ValueError(f"beside a list of inter nets, intra is None or a list of nets, one per member ({G})")
        return self._net_list(as_list, activation, in_dim, out_dim, layout, precision, count=G, per="member", mixed=mixed)

    def _set_population_nets(self, call: str, key: str, G: int, lists, *args):
        with torch.cuda.device(self.device):
            self._check(getattr(self._lib, call)(self._h, G, lists[0][0], lists[1][0] if lists[1] else None, *args, self._stream()), call)
        self._keep[key] = [x[1] for x in lists if x]

    def set_population_member(self, m: int, inter=None, intra=None, v_inter=None, v_intra=None, activation: Optional[str] = None,
                              precision: Optional[Dict[str, str]] = None) -> None:
        """Rebind member ``m``'s copies in place (ranenv_set_population_member): the nets given replace that member's inter actor /
        intra actor / inter critic / intra critic, None leaves a role as it is; shapes as bound -- or, for a role bound with
        ``mixed=True``, any shape whose packed copy fits the member's extent (``population_net``, ``packed_net_floats``).  ``precision``:
        {"policy": ..., "value": ...} as given to the binding calls (default "f32" each).  No other member is touched."""
        G = len(self._population_first()) - 1
        if not 0 <= int(m) < G:
            raise ValueError(f"member {m} outside the population's {G}")
        precision = precision or {}
        layout = NET_IN_OBS if self._intra_layout is None else self._intra_layout
        in_intra = self.W + (self.Us if layout == NET_IN_MASK_OBS else 0)
        keep, structs = [], []
        for net, in_dim, out_dim, lay, prec in ((inter, 10 * self.S, 2 * self.S, NET_IN_OBS, "policy"), (intra, in_intra, 3, layout, "policy"),
                                                (v_inter, 10 * self.S, 1, NET_IN_OBS, "value"), (v_intra, in_intra, 1, layout, "value")):
            if net is None:
                structs.append(None)
                continue
            layers, act = policy_net_layers(net, activation, in_dim, out_dim)
            structs.append(C.byref(self._mlp_struct(layers, act, lay, keep, precision.get(prec, "f32"))))
        with torch.cuda.device(self.device):
            self._check(self._lib.ranenv_set_population_member(self._h, int(m), *structs, self._stream()), "ranenv_set_population_member")
        self._keep.setdefault("population_members", {})[int(m)] = keep

    def population_net(self, role: str, m: int) -> Dict[str, object]:
        """What member ``m`` holds now for ``role`` ("inter", "intra", "v_inter", "v_intra"; ranenv_get_population_net): {"hidden": its
        hidden widths, "dims": [in, hidden..., out], "activation": "tanh" / "relu", "extent": floats of the member's extent in the role's
        buffer, "used": floats of it the net's packed copy takes}."""
        if role not in _lib.POPULATION_ROLES:
            raise ValueError(f"role must be one of {sorted(_lib.POPULATION_ROLES)}")
        G = len(self._population_first()) - 1
        if not 0 <= int(m) < G:
            raise ValueError(f"member {m} outside the population's {G}")
        n_hidden, act, dims, extent, used = C.c_int32(), C.c_int32(), (C.c_int32 * 6)(), C.c_int64(), C.c_int64()
        self._check(self._lib.ranenv_get_population_net(self._h, _lib.POPULATION_ROLES[role], int(m), C.byref(n_hidden), dims, C.byref(act),
                                                        C.byref(extent), C.byref(used)), "ranenv_get_population_net")
        dims = list(dims[:n_hidden.value + 2])
        return {"hidden": dims[1:-1], "dims": dims, "activation": {v: k for k, v in NET_ACTIVATIONS.items()}[act.value], "extent": extent.value,
                "used": used.value}

    packed_net_floats = staticmethod(packed_net_floats)
    ppo_lds_bytes = staticmethod(ppo_lds_bytes)
    ppo_wide_scratch_floats = staticmethod(ppo_wide_scratch_floats)

    def _gae_pairs(self, gamma, lam):
        """``collect`` / ``gae``: None for two scalars, else the members' (gamma [G], lam [G]) as float64 arrays -- a scalar beside a
        sequence stands for every member.  ValueError, before any library call, without a population or for another length than G."""
        seqs = [not np.isscalar(x) and np.ndim(x) > 0 for x in (gamma, lam)]
        if not any(seqs):
            return None
        G = len(self._population_first()) - 1
        out = []
        for name, x, seq in (("gamma", gamma, seqs[0]), ("lam", lam, seqs[1])):
            a = np.asarray(x, dtype=np.float64).reshape(-1) if seq else np.full(G, float(x))
            if a.size != G:
                raise ValueError(f"{name}: {a.size} values given, one per member is {G}")
            out.append(np.ascontiguousarray(a))
        return out

    def evaluate_population(self, n_episodes: int, max_steps=None, per_slice: bool = False) -> Dict[str, np.ndarray]:
        """``evaluate()`` and, per member, the mean of every metric over the member's envs and episodes: {metric: float64 [G]}
        (``"slice"``: [G, S, 10]), plus ``"per_env"``, what ``evaluate()`` returned."""
        first = self._population_first()
        res = self.evaluate(n_episodes, max_steps=max_steps, per_slice=per_slice)
        out = population_means(res, first)
        out["per_env"] = res
        return out

    def set_value_network(self, inter, intra=None, activation: Optional[str] = None, precision: str = "f32", mixed: bool = False):
        """Bind the critics that ``collect()`` evaluates beside the actors (ranenv_set_value_network): ``inter`` maps the
        inter-slice observation [10*S] to one value, ``intra`` (None = no intra critic: those columns of ``vf`` are 0) the
        intra actor's input row -- the layout given to ``set_policy_network`` -- to one value per (env, slice).  Nets as for
        ``policy_net_layers``.  Bind the actors first when there is an intra critic; re-binding either pair leaves the other.
        ``intra`` may be a list of S critics of one shape, ``intra[s]`` for slice index s (ranenv_set_intra_value_networks), with
        shared or per-slice intra actors alike.  ``precision`` as for ``set_policy_network``, for every critic of this call; the
        critics' precision is their own -- bf16 critics beside f32 actors and the reverse are both fine.
        Under ``set_population``, ``inter`` may be a list of G critics (and ``intra`` then None or a list of G), member m's
        (ranenv_set_population_value); population critics beside one actor pair and the reverse are both fine.  ``mixed=True``: the
        members' critics may differ in hidden widths, depth and activation, as for ``set_policy_network`` (ranenv_set_population_value_mixed);
        mixed critics beside uniform actors and the reverse are both fine."""
        layout = lambda layers: NET_IN_MASK_OBS if layers[0][0].shape[1] == self.W + self.Us else NET_IN_OBS  # noqa: E731
        members = per_slice_nets(inter)
        if mixed and members is None:
            raise ValueError("mixed=True takes a list of inter critics, one per member of the population")
        if members is not None:                # a population's critics: inter[m] (and intra[m]) are member m's
            G = self._population_size(len(members))
            lists = [self._net_list(members, activation, 10 * self.S, 1, NET_IN_OBS, precision, count=G, per="member", mixed=mixed),
                     self._member_list(intra, G, activation, None, 1, layout, precision, mixed)]
            if lists[1] is not None and self._intra_layout != lists[1][0][0].contents.input_layout:
                raise ValueError("intra critics read the intra actor's input row: " + (
                    "no intra actor is bound (set_policy_network)" if self._intra_layout is None else "its intra_input is the other layout"))
            self._set_population_nets("ranenv_set_population_value" + ("_mixed" if mixed else ""), "population_value", G, lists)
            for key in ("value_net", "intra_value_nets"):
                self._keep.pop(key, None)
            return
        per_slice = self._net_list(per_slice_nets(intra), activation, None, 1, layout, precision)
        if per_slice is not None and self._intra_layout != per_slice[0][0].contents.input_layout:
            raise ValueError("intra critics per slice read the intra actor's input row: " + (
                "no intra actor is bound (set_policy_network)" if self._intra_layout is None else "its intra_input is the other layout"))
        self._set_nets("value_net", "ranenv_set_value_network", [(inter, activation, 10 * self.S, 1, NET_IN_OBS),
                       (None if per_slice else intra, activation, None, 1, layout)], precision=precision)
        self._set_net_list("intra_value_nets", "ranenv_set_intra_value_networks", per_slice)

    TRAJECTORY_SHAPES = {      # field -> (dtype, slots beyond n_steps, shape of one slot in terms of B, S, Us, W)
        "obs_inter": (torch.float32, 0, lambda B, S, Us, W: (B, 10 * S)), "obs_intra": (torch.float32, 0, lambda B, S, Us, W: (B, S, W)),
        "mask_inter": (torch.int8, 0, lambda B, S, Us, W: (B, S)), "mask_intra": (torch.int8, 0, lambda B, S, Us, W: (B, S, Us)),
        "action_inter": (torch.float64, 0, lambda B, S, Us, W: (B, S)), "action_intra": (torch.uint8, 0, lambda B, S, Us, W: (B, S)),
        "logp": (torch.float32, 0, lambda B, S, Us, W: (B, S + 1)), "vf": (torch.float32, 1, lambda B, S, Us, W: (B, S + 1)),
        "reward": (torch.float64, 0, lambda B, S, Us, W: (B, S + 1)), "done": (torch.uint8, 0, lambda B, S, Us, W: (B,)),
        "adv": (torch.float32, 0, lambda B, S, Us, W: (B, S + 1)), "vtarg": (torch.float32, 0, lambda B, S, Us, W: (B, S + 1)),
    }

    def collect(self, n_steps: int, gamma=0.99, lam=0.95, record=_lib.TRAJECTORY_FIELDS) -> Dict[str, torch.Tensor]:
        """``rollout(n_steps)`` under the policy nets that leaves a PPO batch on the device (ranenv_collect, include/ranenv.h):
        a dict of ``[n_steps, B, ...]`` tensors named as ranenv_trajectory's fields (``vf`` has ``n_steps + 1`` slots, the last
        one the bootstrap value), restricted to ``record``.  ``adv`` / ``vtarg`` are GAE(``gamma``, ``lam``) of the recorded
        ``reward`` / ``vf`` / ``done``.  Needs ``set_policy_network`` and ``set_value_network``.  The tensors are allocated once
        per (n_steps, record) and REUSED: the next ``collect`` of that shape overwrites them.  ``obs_intra`` / ``mask_intra`` /
        ``action_intra`` are only written with an intra actor bound.  The env's state, ``env.reward`` / ``env.done`` / the
        observation buffers and ``policy_actions()`` afterwards are those of ``rollout(n_steps)``.
        Under ``set_population``, ``gamma`` and ``lam`` may each be a sequence of G values, member m's (ranenv_set_population_gae):
        ``adv`` / ``vtarg`` of member m's envs are then GAE(``gamma[m]``, ``lam[m]``)."""
        if self._recorder is not None:
            raise RanEnvError("collect() does not return between TTIs: the recorder needs step()")
        pairs = self._gae_pairs(gamma, lam)
        _pd = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
        if pairs is not None:
            self._check(self._lib.ranenv_set_population_gae(self._h, len(pairs[0]), _pd(pairs[0]), _pd(pairs[1])), "ranenv_set_population_gae")
            gamma, lam = 0.0, 0.0              # (ignored while the members' pairs are set)
        elif getattr(self, "_gae_per_member", False):
            self._check(self._lib.ranenv_set_population_gae(self._h, 0, None, None), "ranenv_set_population_gae")
        self._gae_per_member = pairs is not None
        return self._collect("collect", n_steps, record, _lib.Trajectory, _lib.TRAJECTORY_FIELDS, self.TRAJECTORY_SHAPES, "trajectories",
                             (self.B, self.S, self.Us, self.W), self._lib.ranenv_collect, (float(gamma), float(lam)))

    def _collect(self, name, n_steps, record, struct, fields, shapes, cache_key, sizes, call, args) -> Dict[str, torch.Tensor]:
        """``collect`` / ``collect_head``: the record's tensors (cached per (n_steps, record)), their pointers in ``struct``, the C call."""
        n_steps = int(n_steps)
        traj = struct()
        out: Dict[str, torch.Tensor] = {}
        if n_steps >= 1:
            unknown = set(record) - set(fields)
            if unknown:
                raise ValueError(f"unknown trajectory fields {sorted(unknown)}")
            key = (n_steps, tuple(f for f in fields if f in set(record)))
            cache = self._keep.setdefault(cache_key, {})
            if key not in cache:
                cache[key] = {f: torch.zeros((n_steps + shapes[f][1],) + shapes[f][2](*sizes), dtype=shapes[f][0], device=self.device)
                              for f in key[1]}
            out = cache[key]
            for f, t in out.items():
                setattr(traj, f, t.data_ptr())
        with torch.cuda.device(self.device):
            self._check(call(self._h, n_steps, C.byref(traj), *args, *self._p_out, self._stream()), f"ranenv_{name}")
        return out

    def gae(self, reward: torch.Tensor, vf: torch.Tensor, done: torch.Tensor, gamma=0.99, lam=0.95,
            adv: Optional[torch.Tensor] = None, vtarg: Optional[torch.Tensor] = None):
        """The GAE pass alone (ranenv_gae): ``reward`` float64 [T, B, C], ``vf`` float32 [T + 1, B, C], ``done`` uint8 [T, B] on the
        device -> (``adv``, ``vtarg``) float32 [T, B, C], written into the given tensors or new ones.  ``gamma`` / ``lam``: scalars, or
        under ``set_population`` sequences of G values, member m's for member m's envs (ranenv_gae_population)."""
        pairs = self._gae_pairs(gamma, lam)
        T, B, Cn = reward.shape
        if B != self.B or tuple(vf.shape) != (T + 1, B, Cn) or tuple(done.shape) != (T, B):
            raise RanEnvError(f"gae: reward {tuple(reward.shape)}, vf {tuple(vf.shape)}, done {tuple(done.shape)} do not fit [T, {self.B}, C]")
        reward = self._dev(reward, torch.float64, (T, B, Cn), "reward")
        vf = self._dev(vf, torch.float32, (T + 1, B, Cn), "vf")
        done = self._dev(done, torch.uint8, (T, B), "done")
        adv = torch.empty((T, B, Cn), dtype=torch.float32, device=self.device) if adv is None else self._dev(adv, torch.float32, (T, B, Cn), "adv")
        vtarg = torch.empty((T, B, Cn), dtype=torch.float32, device=self.device) if vtarg is None else self._dev(vtarg, torch.float32, (T, B, Cn), "vtarg")
        if pairs is not None:
            _pd = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
            with torch.cuda.device(self.device):
                self._check(self._lib.ranenv_gae_population(self._h, T, Cn, _ptr(reward), _ptr(vf), _ptr(done), len(pairs[0]), _pd(pairs[0]), _pd(pairs[1]),
                                                            _ptr(adv), _ptr(vtarg), self._stream()), "ranenv_gae_population")
            return adv, vtarg
        with torch.cuda.device(self.device):
            self._check(self._lib.ranenv_gae(self._h, T, Cn, _ptr(reward), _ptr(vf), _ptr(done), float(gamma), float(lam), _ptr(adv), _ptr(vtarg),
                                             self._stream()), "ranenv_gae")
        return adv, vtarg

    # -- the PPO update on the device (ranenv_ppo_bind / ranenv_ppo_update; include/ranenv.h "PPO update") ---------------------------
    PPO_ROW_EPOCHS_CAP, PPO_STEPS_CAP = PPO_ROW_EPOCHS_CAP, PPO_STEPS_CAP      # (per handle: an attribute of the instance overrides them)

    def ppo_bind(self, mixed: bool = False, head: bool = False, wide: bool = False, per_slice: bool = False, spread: bool = False, slabs: Optional[int] = None,
                 bf16: bool = False) -> None:
        """Allocate and zero the optimiser state of the bound actors and critics (ranenv_ppo_bind): Adam moments, gradient scratch,
        one step counter per (member, kind).  Bind the nets first; re-binding a net afterwards restarts its optimiser (see the header).
        ``mixed=True`` (ranenv_ppo_bind_mixed): the population was bound with ``mixed=True`` -- members of differing shape -- and
        ``ppo_update`` trains each member on its own shape; every member's actor / critic pair must fit the LDS plan
        (``ppo_lds_bytes``).  A mixed population is refused without it, a uniform one with it.
        ``head=True`` (ranenv_ppo_bind_head): the state of the head actor, the head critic and ``log_std`` with one step counter, for
        ``ppo_update_head``; it stands beside the IBSched nets' binding.  ``mixed`` and ``head`` exclude each other.
        ``wide=True`` (ranenv_ppo_bind_wide), with or without ``mixed``: the binding for nets beyond the LDS plan, such as the
        reference's ``verybig`` [512, 512, 512] -- two row buffers in LDS and the layers' rows parked in a scratch allocated here
        (``ppo_lds_bytes(..., wide=True)``, ``ppo_wide_scratch_floats``).  Nets that fit both plans train to the same bytes under
        either.  A handle has one binding of the IBSched nets: the later ``ppo_bind`` replaces the earlier one and restarts the
        optimiser.  The head pair trains under the plain plan alone: ``wide`` and ``head`` exclude each other.
        ``per_slice=True`` (ranenv_ppo_bind_slices), with or without ``wide``: the binding for non-shared intra policies -- one inter
        actor and critic, ``intra`` a list of S nets in ``set_policy_network`` and a list of S critics, or none, in
        ``set_value_network`` -- which ``ppo_update_per_slice`` trains, one workgroup per policy.  Every other binding refuses such
        nets.  It excludes ``mixed`` and ``head``.
        ``spread=True`` (ranenv_ppo_bind_spread), with or without ``wide``: the binding for ONE agent on a large batch -- every
        optimiser step of ``ppo_update`` is spread over the chip, the 32-row tiles of a minibatch over up to ``slabs`` (1..256, default 64)
        workgroups per kind, each adding into a gradient slab of its own (``ppo_spread_bytes``); summed in a fixed order, so the
        result depends on the inputs and on min(tiles, slabs) alone.  No population, no nets per slice: it excludes ``mixed``
        and ``per_slice`` -- unless ``slabs`` is given with the latter:
        ``per_slice=True, spread=True, slabs=N`` (ranenv_ppo_bind_slices_spread), with or without ``wide``: the per-slice binding's 1 + S
        policies under the spread schedule -- every optimiser step of ``ppo_update_per_slice`` is three launches in which each policy's
        minibatch is spread over up to ``slabs`` workgroups and slabs of its own (``ppo_slices_spread_bytes`` tells the bytes: they grow
        with S x slabs).  Policy u's bytes are those of ``ppo_bind(spread=True, slabs=N)`` on a handle that holds u's nets as its one
        shared pair and is given u's rows.  ``slabs`` has no default in this form: ``spread`` and ``per_slice`` without it raise
        ``ValueError``, as the two together always did before this form existed.
        ``head=True, spread=True, slabs=N`` (ranenv_ppo_bind_head_spread): the head binding's second form -- every optimiser step of
        ``ppo_update_head`` spread over up to ``slabs`` workgroups in the same three launches, ``log_std`` included
        (``ppo_head_spread_bytes``).  The later of the two head bindings replaces the earlier and restarts the head optimiser; either
        stands beside whatever binding the IBSched nets have, the spread one included.  The head pair trains under the plain LDS plan
        alone: ``head`` with ``spread`` and ``wide`` is refused like ``head`` with ``wide``.  ``slabs`` has no default in this form:
        ``spread`` and ``head`` without it raise ``ValueError``, as the two together always did before this form existed.
        ``spread=True, bf16=True`` (ranenv_ppo_bind_spread_bfloat): the spread binding for nets bound with ``precision="bf16"`` --
        every bound IBSched net must be one --, mixed-precision training: float32 master weights seeded from the acting copy (so
        float32 weights are rounded once, when they are bound), Adam on the masters, and the bf16 acting weights re-rounded from
        them behind every optimiser step, so the next ``collect()`` acts on the trained net (the header's numeric contract;
        ``adapters.ppo_update_reference(..., precision="bf16")`` restates it).  Under it ``net_weights`` returns the masters and
        ``ppo_state`` / ``grad=True`` are in the float32 packed layout.  ``ppo_spread_bf16_bytes`` tells its LDS and device needs.
        Only this binding takes bf16 nets: ``bf16`` needs ``spread`` and excludes ``wide``, ``mixed``, ``per_slice`` and ``head``."""
        if bf16 and not spread:
            raise ValueError("ppo_bind: bf16 needs spread=True (only the one-agent spread binding trains bf16 nets)")
        for other, on in (("wide", wide), ("mixed", mixed), ("per_slice", per_slice), ("head", head)):
            if bf16 and on:
                raise ValueError(f"ppo_bind: bf16 and {other} exclude each other (bf16 nets train under the one-agent spread binding's own LDS plan alone)")
        if spread and mixed:
            raise ValueError("ppo_bind: spread and mixed exclude each other (the spread binding trains one agent, no population)")
        if spread and head and wide:
            raise ValueError("ppo_bind: head, spread and wide exclude each other (the head nets train under the plain plan, spread or not)")
        if spread and per_slice and (slabs is None or head):      # (with slabs: the per-slice binding's spread form, below)
            raise ValueError("ppo_bind: spread and per_slice exclude each other (the spread binding trains one shared intra pair)")
        if per_slice and (mixed or head):
            raise ValueError("ppo_bind: per_slice excludes mixed and head (no population of non-shared agents; the head pair has no slices)")
        if mixed and head:
            raise ValueError("ppo_bind: mixed and head exclude each other")
        if wide and head:
            raise ValueError("ppo_bind: wide and head exclude each other (the head nets train under the plain plan)")
        if spread and head and slabs is None:
            raise ValueError("ppo_bind: spread and head together name the head binding's spread form, which takes its slab count: pass slabs=1..256")
        slabs = 64 if slabs is None else slabs
        with torch.cuda.device(self.device):
            if head and spread:
                self._check(self._lib.ranenv_ppo_bind_head_spread(self._h, int(slabs), self._stream()), "ranenv_ppo_bind_head_spread")
                self._ppo_head_spread = True
                return                         # (beside the IBSched nets' binding: which one that is stays as it was)
            elif bf16:
                self._check(self._lib.ranenv_ppo_bind_spread_bfloat(self._h, int(slabs), self._stream()), "ranenv_ppo_bind_spread_bfloat")
            elif spread and per_slice:
                self._check(self._lib.ranenv_ppo_bind_slices_spread(self._h, int(slabs), 1 if wide else 0, self._stream()), "ranenv_ppo_bind_slices_spread")
            elif spread:
                self._check(self._lib.ranenv_ppo_bind_spread(self._h, int(slabs), 1 if wide else 0, self._stream()), "ranenv_ppo_bind_spread")
            elif per_slice:
                self._check(self._lib.ranenv_ppo_bind_slices(self._h, 1 if wide else 0, self._stream()), "ranenv_ppo_bind_slices")
            elif wide:
                self._check(self._lib.ranenv_ppo_bind_wide(self._h, 1 if mixed else 0, self._stream()), "ranenv_ppo_bind_wide")
            elif head:
                self._check(self._lib.ranenv_ppo_bind_head(self._h, self._stream()), "ranenv_ppo_bind_head")
                self._ppo_head_spread = False
                return                         # (beside the IBSched nets' binding: which one that is stays as it was)
            elif mixed:
                self._check(self._lib.ranenv_ppo_bind_mixed(self._h, self._stream()), "ranenv_ppo_bind_mixed")
            else:
                self._check(self._lib.ranenv_ppo_bind(self._h, self._stream()), "ranenv_ppo_bind")
        self._ppo_spread = bool(spread)
        self._ppo_slices_spread = bool(spread and per_slice)

    def ppo_member_layout(self, m: int, kind: str = "inter") -> Dict[str, int]:
        """What unpacks member ``m``'s block of ``ppo_update(grad=True)["grad"][m, kind]`` (ranenv_ppo_member_layout): the packed
        floats of its "actor" and, behind them, its "critic" (0: none bound) of ``kind`` ("inter" / "intra"), and "lds_bytes", what
        the update of that pair needs.  Under ``ppo_bind(per_slice=True)`` ``m`` is the slice (0 for "inter"): what unpacks row
        ``1 + m`` (row 0) of ``ppo_update_per_slice(grad=True)["grad"]``."""
        if kind not in ("inter", "intra"):
            raise ValueError('kind is "inter" or "intra"')
        a, c, lds = C.c_int64(), C.c_int64(), C.c_int64()
        self._check(self._lib.ranenv_ppo_member_layout(self._h, int(m), 0 if kind == "inter" else 1, C.byref(a), C.byref(c), C.byref(lds)),
                    "ranenv_ppo_member_layout")
        return {"actor": a.value, "critic": c.value, "lds_bytes": lds.value}

    def _ppo_members(self) -> int:
        """Members the update trains: the population's while its inter actors are bound, else 1 (the library's own rule)."""
        if getattr(self, "_population", None) is None:
            return 1
        bound = self._lib.ranenv_get_population_net(self._h, 0, 0, None, None, None, None, None) == 0
        return len(self._population) - 1 if bound else 1

    def ppo_update(self, rec, epochs=10, minibatch=64, lr=3e-4, clip=0.2, vf_coeff=0.5, ent_coeff=0.01, grad_clip=0.5, adv_norm="minibatch",
                   betas=(0.9, 0.999), eps=1e-8, seed=0, order=None, grad: bool = False, probe_logp: bool = False, force: bool = False):
        """Train the bound nets on the ``collect()`` record ``rec`` in one launch (ranenv_ppo_update): per member ``epochs`` passes
        over its rows in shuffled minibatches of ``minibatch`` rows -- clipped-surrogate PPO loss, joint gradient clip, Adam -- written
        in place, so the next ``collect()`` acts on the new weights.  Every hyper-parameter is a scalar or a sequence with one value
        per member of the population (``betas``: one pair for all); ``grad_clip`` <= 0 or None: no clipping; ``adv_norm``:
        "minibatch" (SB3's per-minibatch standardisation) or None (as given: standardise the record's ``adv`` yourself, as RLlib does).
        ``order``: the shuffles as ``adapters.ppo_row_order`` returns them (default: drawn from ``seed``), or "device": drawn from ``seed``
        by ``self.ppo_row_order``, the library's own kernels (other lists than the default's); without "order_intra" only the
        inter nets are trained.  Returns {name: float64 array [G, 2, max epochs]} for the names of ``_lib.PPO_STATS`` (kind 0 inter, 1
        intra); ``grad=True`` adds "grad" [G, 2, floats], the last minibatch's unclipped packed gradient (actor, then critic), and
        ``probe_logp=True`` "logp" [T, B, S + 1], the log-probabilities the update re-evaluated.  A member works on ONE compute unit: more
        than ``PPO_ROW_EPOCHS_CAP`` rows x epochs or ``PPO_STEPS_CAP`` optimiser steps for one member is refused unless ``force`` -- such
        a batch belongs to torch.  Under ``ppo_bind(spread=True)`` the rows are spread over the chip and only ``PPO_STEPS_CAP`` holds
        (a step there is three launches)."""
        G = self._ppo_members()
        hp, epochs, minibatch = ppo_hparams(G, epochs, minibatch, lr, clip, vf_coeff, ent_coeff, grad_clip, adv_norm, betas, eps)
        max_epochs = int(epochs.max())
        if self._device_order(order):
            order = self.ppo_row_order(rec, max(max_epochs, 1), seed, intra=self._intra_layout is not None and "obs_intra" in rec)
        if order is None:
            from .adapters import ppo_row_order
            first_env = self._population if G > 1 else [0, self.B]
            order = ppo_row_order(rec, first_env, max(max_epochs, 1), seed, intra=self._intra_layout is not None and "obs_intra" in rec)
        caps = (PPO_SPREAD_CAPS[0], self.PPO_STEPS_CAP) if getattr(self, "_ppo_spread", False) else (self.PPO_ROW_EPOCHS_CAP, self.PPO_STEPS_CAP)
        firsts = ppo_order_firsts(order, {"inter": G, "intra": G}, epochs, minibatch, caps, "ppo_update", force=force)
        lists, _pi = self._ppo_lists(order, firsts), lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))  # noqa: E731
        return self._ppo_launch("ranenv_ppo_update", lambda T, traj, stats, gbuf, stream: self._lib.ranenv_ppo_update(
            self._h, T, traj, G, hp, _ptr(lists["inter"]), _pi(firsts["inter"]), _ptr(lists.get("intra")), _pi(firsts["intra"]) if "intra" in firsts else None,
            stats, gbuf, stream), rec, (G, 2, max(max_epochs, 1)), (lambda: (G, 2, self._ppo_grad_floats())) if grad else None, probe_logp)

    def _ppo_lists(self, order, firsts):
        """The row lists of the kinds in ``firsts`` as the C call takes them: a list without rows still is a list, not NULL."""
        none = torch.zeros(1, dtype=torch.int32, device=self.device)
        return {k: order["order_" + k] if order["order_" + k].numel() else none for k in firsts}

    def ppo_row_order(self, rec, epochs: int, seed: int = 0, intra: bool = True, per_slice: bool = False) -> Dict[str, object]:
        """``adapters.ppo_row_order``'s dict for the ``collect()`` record ``rec``, drawn by the library's own kernels
        (ranenv_ppo_row_count + ranenv_ppo_row_order, include/ranenv.h "Row lists on the device"): ``order_<kind>`` int32 device tensors
        [epochs, N_kind] and ``first_<kind>`` int32 numpy arrays ("intra": None with ``intra=False``).  The units are the handle's
        population members, or with ``per_slice=True`` (one member only) the one inter agent and the S slices.  A pure function of
        (``rec["mask_inter"]``, grouping, ``seed``, epoch) -- ``adapters.ppo_row_order_reference`` gives the same bytes in numpy, whatever
        the torch build -- and NOT the lists ``adapters.ppo_row_order`` draws from the same seed.  Nothing is sorted; the call waits for
        the device once, for the counts that size the lists."""
        T, B, S = (int(rec["mask_inter"].shape[0]) if "mask_inter" in rec else int(rec["logp"].shape[0])), self.B, self.S
        mask = self._dev(rec["mask_inter"], torch.int8, (T, B, S), "mask_inter") if intra else None
        grouping = _lib.PPO_ROWS_SLICES if per_slice else _lib.PPO_ROWS_MEMBERS
        epochs = int(epochs)
        fi, fa, n = (C.c_int32 * (_lib.POPULATION_MAX + 1))(), (C.c_int32 * (_lib.POPULATION_MAX + 1))(), C.c_int32()
        with torch.cuda.device(self.device):
            self._check(self._lib.ranenv_get_population(self._h, C.byref(n), None), "ranenv_get_population")
            units = {"inter": 1 if per_slice else max(n.value, 1), "intra": S if per_slice else max(n.value, 1)}
            self._check(self._lib.ranenv_ppo_row_count(self._h, T, _ptr(mask), grouping, fi, fa if intra else None, self._stream()), "ranenv_ppo_row_count")
            out = {"order_intra": None, "first_intra": None, "first_inter": np.array(fi[:units["inter"] + 1], dtype=np.int32)}
            out["order_inter"] = torch.empty((max(epochs, 0), int(out["first_inter"][-1])), dtype=torch.int32, device=self.device)
            if intra:
                out["first_intra"] = np.array(fa[:units["intra"] + 1], dtype=np.int32)
                out["order_intra"] = torch.empty((max(epochs, 0), int(out["first_intra"][-1])), dtype=torch.int32, device=self.device)
            lists = [_ptr(o) if o is not None and o.numel() else None for o in (out["order_inter"], out["order_intra"])]
            self._check(self._lib.ranenv_ppo_row_order(self._h, T, _ptr(mask), grouping, epochs, int(seed) & 0xFFFFFFFFFFFFFFFF, lists[0], lists[1],
                                                       self._stream()), "ranenv_ppo_row_order")
        return out

    def ppo_head_row_order(self, rec, epochs: int, seed: int = 0) -> torch.Tensor:
        """The row lists of ``ppo_update_head`` for a ``collect_head()`` record, drawn by the library's own kernels: int32
        [epochs, T * B], per epoch a permutation of the record rows ``t * B + b``.  This is the one-member inter list of
        ``ppo_row_order`` -- equal to ``ppo_row_order(...)["order_inter"]`` for the same seed and record length -- so a handle with a
        population of more than one member is refused.  Not the lists ``adapters.ppo_head_row_order`` draws from the same seed."""
        if getattr(self, "_population", None) is not None and len(self._population) > 2:
            raise RanEnvError("ppo_head_row_order: the head agents' list is the one-member inter list; this handle has a population")
        return self.ppo_row_order(rec, epochs, seed, intra=False)["order_inter"]

    @staticmethod
    def _device_order(order) -> bool:
        """``order="device"`` of the three ``ppo_update*``: the lists come from this handle's ``ppo_row_order`` / ``ppo_head_row_order``."""
        if isinstance(order, str):
            if order != "device":
                raise ValueError(f'order is a dict / tensor of row lists, None (drawn in torch from seed) or "device", not {order!r}')
            return True
        return False

    def _ppo_grad_floats(self) -> int:
        gf = C.c_int64()
        self._check(self._lib.ranenv_ppo_layout(self._h, C.byref(gf), None), "ranenv_ppo_layout")
        return gf.value

    def _ppo_launch(self, name, call, rec, stats_shape, grad_shape=None, probe_logp=False, head=False):
        """What the three ``ppo_update*`` share behind their checks: the record ``rec`` marshalled into a ``Trajectory`` (``head``: a
        ``HeadTrajectory``), the statistics [*stats_shape, len(PPO_STATS)], the gradient buffer of ``grad_shape()`` (None: none) and the
        log-probability buffer of an armed probe, the C ``call(T, traj, stats, grad, stream)`` of ``name``, and the result dict."""
        T = int(rec["logp"].shape[0])
        if head:
            struct, fields, shapes, sizes = _lib.HeadTrajectory, _lib.HEAD_TRAJECTORY_FIELDS, self._head_shapes(self.HEAD_TRAJECTORY_SHAPES, "")[0], (self.B, self.S)
        else:
            struct, fields, shapes, sizes = _lib.Trajectory, _lib.TRAJECTORY_FIELDS, self.TRAJECTORY_SHAPES, (self.B, self.S, self.Us, self.W)
        traj, keep = struct(), []
        for f in fields:
            if f in rec:
                dt, extra, shape = shapes[f]
                keep.append(self._dev(rec[f], dt, (T + extra,) + shape(*sizes), f))
                setattr(traj, f, keep[-1].data_ptr())
        stats = torch.zeros(tuple(stats_shape) + (len(_lib.PPO_STATS),), dtype=torch.float64, device=self.device)
        gbuf = torch.zeros(grad_shape(), dtype=torch.float32, device=self.device) if grad_shape is not None else None
        lbuf = torch.zeros((T, self.B, self.S + 1), dtype=torch.float32, device=self.device) if probe_logp else None
        with torch.cuda.device(self.device):
            if probe_logp:          # (armed for the one update below, which disarms it whether it is served or refused)
                self._check(self._lib.ranenv_ppo_probe_logp(self._h, _ptr(lbuf)), "ranenv_ppo_probe_logp")
            self._check(call(T, C.byref(traj), _ptr(stats), _ptr(gbuf), self._stream()), name)
        host = stats.cpu().numpy()             # (synchronises: the launch is over, `order` and `rec` may go)
        out = {stat: host[..., i] for i, stat in enumerate(_lib.PPO_STATS)}
        if gbuf is not None:
            out["grad"] = gbuf
        if probe_logp:
            out["logp"] = lbuf
        return out

    def ppo_update_per_slice(self, rec, epochs=10, minibatch=64, lr=3e-4, clip=0.2, vf_coeff=0.5, ent_coeff=0.01, grad_clip=0.5, adv_norm="minibatch",
                             betas=(0.9, 0.999), eps=1e-8, seed=0, order=None, grad: bool = False, probe_logp: bool = False, force: bool = False):
        """Train the non-shared IBSched agent on the ``collect()`` record ``rec`` in one launch of 1 + S workgroups
        (ranenv_ppo_update_slices, under ``ppo_bind(per_slice=True)``): the inter pair, and slice s's actor / critic pair on the live
        rows of slice s alone, each with its own Adam state, written in place -- the next ``collect()`` acts on the trained nets.  The
        hyper-parameters are scalars, one set for all 1 + S policies as RLlib's one config; their meaning is ``ppo_update``'s.
        ``order``: as ``adapters.ppo_row_order(..., per_slice=True)`` returns it (default: drawn from ``seed``; "device": drawn from
        ``seed`` by ``self.ppo_row_order(..., per_slice=True)``) -- "first_intra" is
        [S + 1], slice s's share of every epoch's row of "order_intra"; without "order_intra" only the inter pair trains.  Returns
        {name: float64 [1 + S, epochs]} for ``_lib.PPO_STATS``: row 0 the inter pair, row 1 + s slice s (a slice without rows: zeros);
        ``grad=True`` adds "grad" [1 + S, floats] and ``probe_logp=True`` "logp" [T, B, S + 1], as ``ppo_update`` does.
        ``PPO_ROW_EPOCHS_CAP`` and ``PPO_STEPS_CAP`` hold per policy unless ``force``.  Under ``ppo_bind(per_slice=True, spread=True,
        slabs=N)`` every optimiser step is three launches spread over the chip: the rows x epochs cap does not apply, ``PPO_STEPS_CAP``
        does, per policy."""
        if adv_norm not in ("minibatch", "none", None):
            raise ValueError('adv_norm is "minibatch" or None')
        for name, x in (("epochs", epochs), ("minibatch", minibatch), ("lr", lr), ("clip", clip), ("vf_coeff", vf_coeff), ("ent_coeff", ent_coeff),
                        ("grad_clip", 0.0 if grad_clip is None else grad_clip), ("eps", eps)):
            if np.ndim(x) != 0:
                raise ValueError(f"{name}: ppo_update_per_slice takes one value for all policies")
        hp, epochs, minibatch = ppo_hparams(1, epochs, minibatch, lr, clip, vf_coeff, ent_coeff, grad_clip, adv_norm, betas, eps)
        max_epochs, S = int(epochs[0]), self.S
        if self._device_order(order):
            order = self.ppo_row_order(rec, max(max_epochs, 1), seed, intra=self._intra_layout is not None and "obs_intra" in rec, per_slice=True)
        if order is None:
            from .adapters import ppo_row_order
            order = ppo_row_order(rec, [0, self.B], max(max_epochs, 1), seed, intra=self._intra_layout is not None and "obs_intra" in rec, per_slice=True)
        caps = (PPO_SPREAD_CAPS[0], self.PPO_STEPS_CAP) if getattr(self, "_ppo_slices_spread", False) else (self.PPO_ROW_EPOCHS_CAP, self.PPO_STEPS_CAP)
        firsts = ppo_order_firsts(order, {"inter": 1, "intra": S}, epochs, minibatch, caps, "ppo_update_per_slice", per_slice=True, force=force)
        lists = self._ppo_lists(order, firsts)
        return self._ppo_launch("ranenv_ppo_update_slices", lambda T, traj, stats, gbuf, stream: self._lib.ranenv_ppo_update_slices(
            self._h, T, traj, hp, _ptr(lists["inter"]), int(firsts["inter"][1]), _ptr(lists.get("intra")),
            firsts["intra"].ctypes.data_as(C.POINTER(C.c_int32)) if "intra" in firsts else None, stats, gbuf, stream),
            rec, (1 + S, max(max_epochs, 1)), (lambda: (1 + S, self._ppo_grad_floats())) if grad else None, probe_logp)

    _NET_ROLES = {"inter": 0, "intra": 1, "v_inter": 2, "v_intra": 3}

    def net_weights(self, role: str, m: int = 0, slice: Optional[int] = None):
        """The bound float32 net of ``role`` ("inter", "intra", "v_inter", "v_intra"), member ``m`` of a population, as it is on the
        device NOW -- after ``ppo_update``: the trained net -- as a list of ``(W, b)`` tensors in torch ``Linear`` layout
        (ranenv_get_net_weights); with ``net_activation(role, m)`` what ``set_policy_network`` takes.  ``slice=s``: slice s's net of
        "intra" / "v_intra" bound per slice (ranenv_get_slice_net_weights), which ``m`` cannot name.  A bf16 net has no float32 weights
        to return -- they were rounded at bind -- except under ``ppo_bind(spread=True, bf16=True)``: then these are the float32 MASTER
        weights the optimiser steps, of which the acting copy is the bf16 rounding."""
        layers, _ = self._net_weights(role, m, slice=slice)
        return layers

    def net_activation(self, role: str, m: int = 0, slice: Optional[int] = None) -> str:
        return self._net_weights(role, m, copy=False, slice=slice)[1]

    def _net_weights(self, role: str, m: int, copy: bool = True, slice: Optional[int] = None):
        if role not in self._NET_ROLES:
            raise ValueError(f"role must be one of {sorted(self._NET_ROLES)}")
        call, m = ("ranenv_get_net_weights", m) if slice is None else ("ranenv_get_slice_net_weights", slice)
        return self._export_net(call, self._NET_ROLES[role], int(m), copy=copy)

    def _export_net(self, call: str, *ids, copy: bool = True):
        """The two-call export behind ``net_weights`` / ``head_net_weights`` / ``sac_net_weights``: ``call(handle, *ids, mlp, stream)``
        once for the net's shape, then again with ``(W, b)`` tensors of that shape to fill -> (layers, activation)."""
        out = _lib.Mlp()
        with torch.cuda.device(self.device):
            self._check(getattr(self._lib, call)(self._h, *ids, C.byref(out), self._stream()), call)
            act = {v: k for k, v in NET_ACTIVATIONS.items()}[out.activation]
            if not copy:
                return None, act
            dims = list(out.dims[:out.n_hidden + 2])
            layers = [(torch.empty((dims[i + 1], dims[i]), dtype=torch.float32, device=self.device),
                       torch.empty((dims[i + 1],), dtype=torch.float32, device=self.device)) for i in range(len(dims) - 1)]
            for i, (w, b) in enumerate(layers):
                out.weight[i], out.bias[i] = w.data_ptr(), b.data_ptr()
            self._check(getattr(self._lib, call)(self._h, *ids, C.byref(out), self._stream()), call)
        return layers, act

    def _opt_views(self, call: str, *ids) -> Dict[str, torch.Tensor]:
        """``ppo_state`` / ``ppo_head_state`` / ``sac_state``: zero-copy views of what ``call(handle, *ids, &m, &v, &t, &floats)`` points at."""
        pm, pv, pt, n = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_int64()
        self._check(getattr(self._lib, call)(self._h, *ids, C.byref(pm), C.byref(pv), C.byref(pt), C.byref(n)), call)
        return {"m": torch.as_tensor(_DevArray(pm.value, (n.value,), "f4", self), device=self.device),
                "v": torch.as_tensor(_DevArray(pv.value, (n.value,), "f4", self), device=self.device),
                "t": torch.as_tensor(_DevArray(pt.value, (1,), "i4", self), device=self.device)}

    def ppo_state(self, role: str, m: int = 0, slice: Optional[int] = None) -> Dict[str, torch.Tensor]:
        """Zero-copy views of the optimiser state of ``role``'s net of member ``m`` (ranenv_ppo_state): Adam's "m" and "v" in the packed
        layout (float32 [floats]) and "t", the (member, kind) step counter (int32 [1]).  ``slice=s``: under ``ppo_bind(per_slice=True)``
        (ranenv_ppo_slice_state) slice s's net of "intra" / "v_intra" with that slice's counter; "inter" / "v_inter" ignore ``s``."""
        call, m = ("ranenv_ppo_state", m) if slice is None else ("ranenv_ppo_slice_state", slice)
        return self._opt_views(call, self._NET_ROLES[role], int(m))

    # -- the learned baselines SchedTWC / SchedColORAN (RANENV_POLICY_HEAD_NETWORK) ------------------------------------------------
    def set_head_policy_network(self, actor, dist: str = "gauss_clip", log_std=None, stochastic: bool = False, seed: int = 0,
                                activation: Optional[str] = None, allow_sorted: bool = False, fixed_intra: Optional[int] = None,
                                observation: str = "head", precision: str = "f32"):
        """Run a trained SchedTWC / SchedColORAN actor on the device in front of every TTI (RANENV_POLICY_HEAD_NETWORK,
        include/ranenv.h): ``actor`` maps ``head_obs`` [10*S] to S outputs (``dist`` "gauss_clip": SB3 PPO, the mean; ``log_std``
        [S] is the policy's parameter) or 2*S outputs ("gauss_tanh": SB3 SAC, (mu | log_std); ``log_std`` must be None).  Nets as
        for ``policy_net_layers`` (``activation`` default: tanh for gauss_clip, relu for gauss_tanh -- SB3's).  Needs
        ``enable_heads()``.  Switches the policy to HEAD_NETWORK with round-robin inside the slices (``fixed_intra``: another).
        SchedTWC runs IBSched without slice sorting (sched_twc.py:75-82): scenario tables whose ``sorted_slices`` is not the
        identity raise RanEnvError unless ``allow_sorted``.
        ``observation`` "inter" (ranenv_set_head_policy_source): the reference's IBSchedSB3, ``sb3_sched`` -- and with
        ``fixed_intra=INTRA_PF`` ``sb3_pf_sched`` --, the same SB3 actor on IBSched's own player_0 observation: it reads ``obs_inter``
        (slices in sorted positions, IBSched's default: no ``allow_sorted`` check), needs no ``enable_heads()``, and ``collect_head`` /
        the replay ring record the step's ``[S + 1]`` reward rows, whose column 0 (``reward="ibsched"``) is its reward.  The source
        in force is ``self.head_observation``; changing it unbinds a bound replay ring.
        ``precision`` as for ``set_policy_network``.  ``sac_targets()`` needs an f32 actor: training targets stay float32."""
        if observation not in HEAD_SOURCES:
            raise ValueError(f"observation must be one of {sorted(HEAD_SOURCES)}")
        if dist not in HEAD_DISTS:
            raise ValueError(f"dist must be one of {sorted(HEAD_DISTS)}")
        inter = observation == "inter"
        if not inter and getattr(self, "head_obs", None) is None:
            raise RanEnvError("set_head_policy_network needs enable_heads(): the actor reads head_obs")
        if self.tables is not None and not allow_sorted and not inter:
            ss = np.asarray(self.tables.sorted_slices)
            if not np.array_equal(ss, np.broadcast_to(np.arange(ss.shape[-1]), ss.shape)):
                raise RanEnvError("the scenario tables sort the slices; SchedTWC / SchedColORAN run with enable_sort_slices=False "
                                  "(pass allow_sorted=True to run the head policy on sorted positions anyway)")
        if (dist == "gauss_clip") != (log_std is not None):
            raise ValueError("log_std is required for gauss_clip and must be None for gauss_tanh")
        if activation is None and not isinstance(actor, torch.nn.Module):
            activation = "tanh" if dist == "gauss_clip" else "relu"
        ls = None
        if log_std is not None:
            ls = torch.as_tensor(log_std).detach().to(device=self.device, dtype=torch.float32).contiguous()
            if tuple(ls.shape) != (self.S,):
                raise ValueError(f"log_std: expected shape ({self.S},), got {tuple(ls.shape)}")
        self._set_nets("head_policy_net", "ranenv_set_head_policy_network",
                       [(actor, activation, 10 * self.S, self.S if dist == "gauss_clip" else 2 * self.S, NET_IN_OBS)],
                       HEAD_DISTS[dist], _ptr(ls), 1 if stochastic else 0, int(seed) & (2 ** 64 - 1), keep=[ls], precision=precision)
        self._policy_views = None
        self._check(self._lib.ranenv_set_head_policy_source(self._h, HEAD_SOURCES[observation]), "ranenv_set_head_policy_source")
        if observation != self.head_observation:
            self._keep.pop("replay", None)         # (the library has unbound the ring: its reward rows change width)
        self.head_observation = observation
        self.set_policy(POLICY_HEAD_NETWORK, INTRA_RR if fixed_intra is None else fixed_intra)

    def set_head_value_network(self, critic, activation: Optional[str] = None, precision: str = "f32"):
        """Bind the critic ``collect_head()`` evaluates beside the head actor (ranenv_set_head_value_network): ``head_obs`` [10*S]
        (``obs_inter`` under the head policy source "inter") -> one value.  Nets as for ``policy_net_layers``; ``precision`` as
        for ``set_policy_network``."""
        self._set_nets("head_value_net", "ranenv_set_head_value_network", [(critic, activation, 10 * self.S, 1, NET_IN_OBS)],
                       precision=precision)

    HEAD_TRAJECTORY_SHAPES = {     # field -> (dtype, slots beyond n_steps, shape of one slot in terms of B, S)
        "obs_head": (torch.float32, 0, lambda B, S: (B, 10 * S)), "action": (torch.float64, 0, lambda B, S: (B, S)),
        "logp": (torch.float32, 0, lambda B, S: (B,)), "vf": (torch.float32, 1, lambda B, S: (B,)),
        "reward_head": (torch.float64, 0, lambda B, S: (B, 2)), "done": (torch.uint8, 0, lambda B, S: (B,)),
        "adv": (torch.float32, 0, lambda B, S: (B,)), "vtarg": (torch.float32, 0, lambda B, S: (B,)),
    }

    def _head_shapes(self, shapes, cache_key):
        """A head record's / ring's shapes under the source in force: "inter" widens ``reward_head`` to the step's [S + 1] row."""
        if self.head_observation != "inter":
            return shapes, cache_key
        wide = dict(shapes)
        wide["reward_head"] = shapes["reward_head"][:-1] + (lambda B, S: (B, S + 1),)
        return wide, "inter_" + cache_key

    def collect_head(self, n_steps: int, reward: Optional[str] = None, gamma: float = 0.99, lam: float = 0.95,
                     record=_lib.HEAD_TRAJECTORY_FIELDS) -> Dict[str, torch.Tensor]:
        """``rollout(n_steps)`` under the head actor that leaves a PPO batch on the device (ranenv_collect_head, include/ranenv.h):
        a dict of ``[n_steps, B, ...]`` tensors named as ranenv_head_trajectory's fields (``vf`` has ``n_steps + 1`` slots),
        restricted to ``record``.  ``adv`` / ``vtarg`` are GAE(``gamma``, ``lam``) on the ``reward`` column ("twc" / "colran"; None =
        "twc") of ``reward_head``.  Under the head policy source "inter" ``obs_head`` holds the ``obs_inter`` rows, ``reward_head`` is
        the step's ``[n_steps, B, S + 1]`` rows and ``reward`` is "ibsched" (column 0; None = that); a name of the other source raises.  Needs a "gauss_clip" ``set_head_policy_network`` and ``set_head_value_network``.  The tensors are
        allocated once per (n_steps, record) and REUSED.  Everything else afterwards is as after ``rollout(n_steps)``."""
        if self._recorder is not None:
            raise RanEnvError("collect_head() does not return between TTIs: the recorder needs step()")
        col = head_reward_column(self.head_observation, reward)
        shapes, cache_key = self._head_shapes(self.HEAD_TRAJECTORY_SHAPES, "head_trajectories")
        return self._collect("collect_head", n_steps, record, _lib.HeadTrajectory, _lib.HEAD_TRAJECTORY_FIELDS, shapes,
                             cache_key, (self.B, self.S), self._lib.ranenv_collect_head, (col, float(gamma), float(lam)))

    # -- the PPO update of the head policies (ranenv_ppo_bind_head / ranenv_ppo_update_head; include/ranenv.h) ----------------------
    def ppo_update_head(self, rec, epochs=10, minibatch=64, lr=3e-4, clip=0.2, vf_coeff=0.5, ent_coeff=0.0, grad_clip=0.5, adv_norm="minibatch",
                        betas=(0.9, 0.999), eps=1e-5, seed=0, order=None, grad: bool = False, force: bool = False):
        """Train the head actor, the head critic and ``log_std`` on the ``collect_head()`` record ``rec`` in one launch of one workgroup
        (ranenv_ppo_update_head): SB3's ``PPO.train`` with ``clip_range_vf=None`` -- the defaults are SB3's -- written in place, so the
        next ``collect_head()`` acts on the trained policy.  ``order``: int32 [>= epochs, n_rows] record rows ``t * B + b`` (default:
        ``adapters.ppo_head_row_order(rec, epochs, seed)``; "device": ``self.ppo_head_row_order(rec, epochs, seed)``).  ``adv_norm``: "minibatch" or None; ``grad_clip`` <= 0 or None: no clipping.
        Returns {name: float64 array [max epochs]} for the names of ``_lib.PPO_STATS``; ``grad=True`` adds "grad" [actor floats + critic
        floats + S], the last minibatch's unclipped gradient: actor packed, critic packed, ``log_std``.  More than ``PPO_ROW_EPOCHS_CAP``
        rows x epochs or ``PPO_STEPS_CAP`` optimiser steps is refused unless ``force``: one compute unit works through them.  Under
        ``ppo_bind(head=True, spread=True)`` every optimiser step is three launches spread over the chip: the rows x epochs cap does not
        apply, ``PPO_STEPS_CAP`` does."""
        if adv_norm not in ("minibatch", "none", None):
            raise ValueError('adv_norm is "minibatch" or None')
        epochs, minibatch = int(epochs), int(minibatch)
        if self._device_order(order):
            order = self.ppo_head_row_order(rec, max(epochs, 1), seed)
        if order is None:
            from .adapters import ppo_head_row_order
            order = ppo_head_row_order(rec, max(epochs, 1), seed)
        if order.dtype != torch.int32 or order.dim() != 2 or order.shape[0] < epochs or not order.is_contiguous():
            raise ValueError(f"order: contiguous int32 [>= {epochs} epochs, n_rows]")
        order = order.to(self.device)
        max_epochs, n_rows = int(order.shape[0]), int(order.shape[1])
        if not force and not getattr(self, "_ppo_head_spread", False) and n_rows * max(epochs, 0) > self.PPO_ROW_EPOCHS_CAP:
            raise RanEnvError(f"ppo_update_head: more than {self.PPO_ROW_EPOCHS_CAP} rows x epochs; one compute unit works through them -- "
                              "train such a batch in torch, or pass force=True")
        steps = -(-n_rows // max(minibatch, 1)) * max(epochs, 0)
        if not force and steps > self.PPO_STEPS_CAP:
            raise RanEnvError(f"ppo_update_head: more than {self.PPO_STEPS_CAP} optimiser steps ({steps}); every step passes over all "
                              "parameters" + (" in three launches" if getattr(self, "_ppo_head_spread", False) else " on one compute unit") +
                              " -- use larger minibatches or fewer epochs, or pass force=True")
        lr, clip, vf_coeff, ent_coeff, eps = float(lr), float(clip), float(vf_coeff), float(ent_coeff), float(eps)      # (one value each)
        hp, _, _ = ppo_hparams(1, epochs, minibatch, lr, clip, vf_coeff, ent_coeff, None if grad_clip is None else float(grad_clip), adv_norm, betas, eps)

        def grad_shape():
            a, c = C.c_int64(), C.c_int64()
            self._check(self._lib.ranenv_ppo_head_layout(self._h, C.byref(a), C.byref(c), None), "ranenv_ppo_head_layout")
            return (a.value + c.value + self.S,)
        none = torch.zeros(1, dtype=torch.int32, device=self.device)      # (a list without rows still is a list: not NULL)
        out = self._ppo_launch("ranenv_ppo_update_head", lambda T, traj, stats, gbuf, stream: self._lib.ranenv_ppo_update_head(
            self._h, T, traj, hp, _ptr(order if order.numel() else none), n_rows, max_epochs, stats, gbuf, stream),
            rec, (max(max_epochs, 1),), grad_shape if grad else None, head=True)
        return {k: v if k == "grad" else v[:max_epochs] for k, v in out.items()}

    def ppo_head_layout(self) -> Dict[str, int]:
        """The packed floats of the head "actor" and "critic" -- the layout of ``ppo_update_head(grad=True)["grad"]``, ``log_std`` [S]
        behind them -- and "lds_bytes" of the launch (ranenv_ppo_head_layout)."""
        a, c, lds = C.c_int64(), C.c_int64(), C.c_int64()
        self._check(self._lib.ranenv_ppo_head_layout(self._h, C.byref(a), C.byref(c), C.byref(lds)), "ranenv_ppo_head_layout")
        return {"actor": a.value, "critic": c.value, "lds_bytes": lds.value}

    _HEAD_NETS = {"actor": 0, "critic": 1, "log_std": 2}

    def head_net_weights(self, which: str):
        """The head "actor" or "critic" as it is on the device NOW -- after ``ppo_update_head``: the trained net -- as a list of
        ``(W, b)`` tensors in torch ``Linear`` layout (ranenv_get_head_net_weights)."""
        if which not in ("actor", "critic"):
            raise ValueError('which is "actor" or "critic"')
        return self._export_net("ranenv_get_head_net_weights", self._HEAD_NETS[which])[0]

    def head_log_std(self) -> torch.Tensor:
        """A copy of the handle's ``log_std`` float32 [S] as it is NOW (ranenv_get_head_log_std)."""
        out = torch.empty((self.S,), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            self._check(self._lib.ranenv_get_head_log_std(self._h, _ptr(out), self._stream()), "ranenv_get_head_log_std")
        return out

    def ppo_head_state(self, which: str) -> Dict[str, torch.Tensor]:
        """Zero-copy views of the optimiser state of the head "actor", "critic" (packed layout) or "log_std" ([S]): Adam's "m" and "v"
        and "t", the one step counter (ranenv_ppo_head_state)."""
        if which not in self._HEAD_NETS:
            raise ValueError(f"which must be one of {sorted(self._HEAD_NETS)}")
        return self._opt_views("ranenv_ppo_head_state", self._HEAD_NETS[which])

    # -- off-policy (SAC) collection: replay ring, sampler, targets (include/ranenv.h "Off-policy collection") ----------------------
    REPLAY_SHAPES = {          # field -> (dtype, shape of one slot in terms of B, S)
        "obs": (torch.float32, lambda B, S: (B, 10 * S)), "next_obs": (torch.float32, lambda B, S: (B, 10 * S)),
        "action": (torch.float64, lambda B, S: (B, S)), "reward_head": (torch.float64, lambda B, S: (B, 2)),
        "done": (torch.uint8, lambda B, S: (B,)),
    }

    def bind_replay(self, capacity: int) -> Dict[str, torch.Tensor]:
        """Allocate and bind a replay ring of ``capacity`` TTIs (ranenv_bind_replay): a dict of ``[capacity, B, ...]`` tensors
        ``obs`` / ``next_obs`` float32 [.., 10*S], ``action`` float64 [.., S] (the score the step consumed), ``reward_head`` float64
        [.., 2] (under the head policy source "inter": [.., S + 1], the step's reward rows, and ``obs`` / ``next_obs`` hold ``obs_inter``
        rows), ``done`` uint8.  The k-th TTI recorded since binding goes to slot ``k % capacity``; binding zeroes the count."""
        capacity = int(capacity)
        shapes, _ = self._head_shapes(self.REPLAY_SHAPES, "")
        ring = {f: torch.zeros((max(capacity, 0),) + shape(self.B, self.S), dtype=dt, device=self.device) for f, (dt, shape) in shapes.items()}
        st = _lib.Replay()
        st.capacity = capacity
        for f, t in ring.items():
            setattr(st, f, t.data_ptr())
        self._check(self._lib.ranenv_bind_replay(self._h, C.byref(st)), "ranenv_bind_replay")
        self._keep["replay"] = ring
        return ring

    def unbind_replay(self) -> None:
        self._check(self._lib.ranenv_bind_replay(self._h, None), "ranenv_bind_replay")
        self._keep.pop("replay", None)

    def collect_replay(self, n_steps: int):
        """``rollout(n_steps)`` under the head actor (either dist) that records every TTI into the bound replay ring
        (ranenv_collect_replay); ``n_steps`` may not exceed the ring's capacity.  Everything else afterwards is as after
        ``rollout(n_steps)``.  Returns the last TTI's (obs, reward, done)."""
        if self._recorder is not None:
            raise RanEnvError("collect_replay() does not return between TTIs: the recorder needs step()")
        with torch.cuda.device(self.device):
            self._check(self._lib.ranenv_collect_replay(self._h, int(n_steps), *self._p_out, self._stream()), "ranenv_collect_replay")
        return self._obs(), self.reward, self.done

    def replay_count(self) -> int:
        """TTIs recorded into the ring since ``bind_replay`` (ranenv_get_replay_count)."""
        n = C.c_int64()
        self._check(self._lib.ranenv_get_replay_count(self._h, C.byref(n)), "ranenv_get_replay_count")
        return int(n.value)

    def replay_sample(self, n: int, seed: int = 0, draw: int = 0, reward: Optional[str] = None) -> Dict[str, torch.Tensor]:
        """``n`` transitions drawn uniformly from the filled part of the ring (ranenv_replay_sample), in the learner's dtypes: ``obs``
        / ``next_obs`` float32 [n, 10*S], ``action`` float32 [n, S], ``reward`` float32 [n] (column "twc" / "colran" of
        ``reward_head``; under the head policy source "inter": "ibsched", column 0; None = the source's first), ``done`` uint8 [n], ``index`` int64 [n] (slot * B + env).  A function of (``seed``, ``draw``, the fill)
        alone.  The tensors are allocated once per ``n`` and REUSED."""
        col = head_reward_column(self.head_observation, reward)
        n = int(n)
        cache = self._keep.setdefault("replay_samples", {})
        if n >= 1 and n not in cache:
            f32 = dict(dtype=torch.float32, device=self.device)
            cache[n] = {"obs": torch.zeros((n, 10 * self.S), **f32), "action": torch.zeros((n, self.S), **f32), "reward": torch.zeros(n, **f32),
                        "next_obs": torch.zeros((n, 10 * self.S), **f32), "done": torch.zeros(n, dtype=torch.uint8, device=self.device),
                        "index": torch.zeros(n, dtype=torch.int64, device=self.device)}
        out = cache.get(n, {})
        m64 = 2 ** 64 - 1
        with torch.cuda.device(self.device):
            self._check(self._lib.ranenv_replay_sample(self._h, n, int(seed) & m64, int(draw) & m64, col,
                                                       *(_ptr(out.get(f)) for f in ("obs", "action", "reward", "next_obs", "done", "index")),
                                                       self._stream()), "ranenv_replay_sample")
        return out

    def set_sac_critics(self, q1, q2, activation: Optional[str] = None):
        """Bind SAC's two Q-nets -- the learner's TARGET critics -- for ``sac_targets()`` (ranenv_set_sac_critics): each maps
        ``[obs (10*S) | action (S)]`` to one value; both of one shape.  Nets as for ``policy_net_layers`` (lists of (W, b):
        ``activation`` default relu, SB3's for SAC).  Re-binding them leaves the actor as it is and vice versa."""
        self._set_nets("sac_critics", "ranenv_set_sac_critics", [
            (q, activation if activation is not None or isinstance(q, torch.nn.Module) else "relu", 11 * self.S, 1, NET_IN_OBS) for q in (q1, q2)])

    def sac_targets(self, next_obs, reward, done, gamma: float = 0.99, ent_coef: float = 0.0, stochastic: bool = True, seed: int = 0,
                    draw: int = 0, outputs=("target", "next_action", "next_logp", "q")) -> Dict[str, torch.Tensor]:
        """SAC's soft Bellman target of ``n`` rows on the device (ranenv_sac_targets): ``next_obs`` float32 [n, 10*S], ``reward``
        float32 [n], ``done`` uint8 [n] -- a ``replay_sample()`` or any other rows -- under the bound "gauss_tanh" head actor and
        ``set_sac_critics``: a' ~ pi(.|next_obs), ``target`` = reward + gamma (1 - done) (min(Q1, Q2)(next_obs, a') - ent_coef
        log pi(a')).  Returns new float32 tensors ``target`` [n], ``next_action`` [n, S], ``next_logp`` [n], ``q`` [n, 2]
        (restricted to ``outputs``; ``target`` always).  The noise is a function of (``seed``, ``draw``, row)."""
        n = int(next_obs.shape[0])
        next_obs = self._dev(next_obs, torch.float32, (n, 10 * self.S), "next_obs")
        reward = self._dev(reward, torch.float32, (n,), "reward")
        done = self._dev(done, torch.uint8, (n,), "done")
        shapes = {"target": (n,), "next_action": (n, self.S), "next_logp": (n,), "q": (n, 2)}
        unknown = set(outputs) - set(shapes)
        if unknown:
            raise ValueError(f"unknown outputs {sorted(unknown)}")
        out = {f: torch.empty(shapes[f], dtype=torch.float32, device=self.device) for f in shapes if f == "target" or f in set(outputs)}
        m64 = 2 ** 64 - 1
        with torch.cuda.device(self.device):
            self._check(self._lib.ranenv_sac_targets(self._h, n, _ptr(next_obs), _ptr(reward), _ptr(done), float(gamma), float(ent_coef),
                                                     1 if stochastic else 0, int(seed) & m64, int(draw) & m64,
                                                     *(_ptr(out.get(f)) for f in ("target", "next_action", "next_logp", "q")), self._stream()),
                        "ranenv_sac_targets")
        return out

    # -- the SAC update (ranenv_sac_bind / ranenv_sac_update; include/ranenv.h "SAC update") ---------------------------------------------
    sac_lds_bytes = staticmethod(sac_lds_bytes)

    def sac_bind(self, ent_coef="auto", target_entropy: Optional[float] = None, slabs: int = 32) -> None:
        """Bind the learner state of SB3's SAC to the bound "gauss_tanh" head actor and the ``set_sac_critics`` pair (ranenv_sac_bind):
        two LIVE critics that start as copies of the bound (target) critics, Adam's moments and counters at zero, the entropy
        coefficient, ``slabs`` gradient slabs (1..256: the most workgroups a pass spreads a minibatch's 32-row tiles over).
        ``ent_coef``: "auto" (trained from 1.0, SB3's default), "auto_0.1" (trained from that value) or a float (fixed).
        ``target_entropy`` None: -S, SB3's default for a Box action space."""
        auto, init = 0, 1.0
        if isinstance(ent_coef, str):
            if not ent_coef.startswith("auto"):
                raise ValueError('ent_coef is "auto", "auto_<initial value>" or a float')
            auto = 1
            if "_" in ent_coef:
                init = float(ent_coef.split("_")[1])
        else:
            init = float(ent_coef)
        te = -float(self.S) if target_entropy is None else float(target_entropy)
        with torch.cuda.device(self.device):
            self._check(self._lib.ranenv_sac_bind(self._h, init, auto, te, int(slabs), self._stream()), "ranenv_sac_bind")

    def sac_layout(self) -> Dict[str, int]:
        """The packed floats of the "actor" and of one "critic" -- ``sac_update(grad=True)["grad"]`` is [actor | q1 | q2 |
        log_ent_coef] -- and "lds_bytes" of the passes (ranenv_sac_layout)."""
        a, c, lds = C.c_int64(), C.c_int64(), C.c_int64()
        self._check(self._lib.ranenv_sac_layout(self._h, C.byref(a), C.byref(c), C.byref(lds)), "ranenv_sac_layout")
        return {"actor": a.value, "critic": c.value, "lds_bytes": lds.value}

    def sac_update(self, batch, steps: int, minibatch: int = 256, lr: float = 3e-4, gamma: float = 0.99, tau: float = 0.005, seed: int = 0,
                   draw: int = 0, first_row: int = 0, grad: bool = False, target: bool = False) -> Dict[str, object]:
        """``steps`` gradient steps of SB3's ``SAC.train`` on the device (ranenv_sac_update; the defaults are SB3's): step g takes rows
        ``[g * minibatch, (g + 1) * minibatch)`` of ``batch`` -- a ``replay_sample(steps * minibatch)`` or any dict of ``obs`` /
        ``next_obs`` float32 [n, 10*S], ``action`` float32 [n, S], ``reward`` float32 [n], ``done`` uint8 [n] with at least that many
        rows -- and updates in place the live critics, the head actor (the next ``collect_replay()`` acts on it), the entropy
        coefficient and the bound target critics (``sac_targets()`` reads them).  Row k of step g draws its noise at the global index
        ``first_row + g * minibatch + k`` under (``seed``, ``draw``).  Returns {name: float64 array [steps]} for ``_lib.SAC_STATS``;
        ``grad=True`` adds "grad", the LAST step's float32 [actor | q1 | q2 | log_ent_coef] in the packed layouts (``sac_layout``);
        ``target=True`` adds "target" float32 [steps * minibatch], every step's soft Bellman targets."""
        steps, minibatch = int(steps), int(minibatch)
        n = max(steps, 0) * max(minibatch, 0)
        rows = {"obs": (torch.float32, (10 * self.S,)), "action": (torch.float32, (self.S,)), "reward": (torch.float32, ()),
                "next_obs": (torch.float32, (10 * self.S,)), "done": (torch.uint8, ())}
        dev = {}
        for f, (dt, tail) in rows.items():
            t = batch[f]
            if t.shape[0] < n:
                raise ValueError(f"batch[{f!r}] has {t.shape[0]} rows, {steps} steps of {minibatch} need {n}")
            dev[f] = self._dev(t, dt, (t.shape[0],) + tail, f)
        stats = torch.zeros((max(steps, 1), len(_lib.SAC_STATS)), dtype=torch.float64, device=self.device)
        gbuf = tbuf = None
        if grad:
            lay = self.sac_layout()
            gbuf = torch.zeros((lay["actor"] + 2 * lay["critic"] + 1,), dtype=torch.float32, device=self.device)
        if target:
            tbuf = torch.zeros((max(n, 1),), dtype=torch.float32, device=self.device)
        m64 = 2 ** 64 - 1
        with torch.cuda.device(self.device):
            self._check(self._lib.ranenv_sac_update(self._h, steps, minibatch, int(first_row), *(_ptr(dev[f]) for f in rows), float(lr), float(gamma),
                                                    float(tau), int(seed) & m64, int(draw) & m64, _ptr(stats), _ptr(gbuf), _ptr(tbuf), self._stream()),
                        "ranenv_sac_update")
        host = stats.cpu().numpy()             # (synchronises: the launches are over, the batch may go)
        out = {name: host[:steps, i] for i, name in enumerate(_lib.SAC_STATS)}
        if grad:
            out["grad"] = gbuf
        if target:
            out["target"] = tbuf[:n]
        return out

    def sac_net_weights(self, which: str):
        """One of the SAC binding's nets as it is on the device NOW, as a list of ``(W, b)`` tensors in torch ``Linear`` layout
        (ranenv_get_sac_net_weights): "actor" (the head actor), "q1" / "q2" (the live critics), "q1_target" / "q2_target" (the bound
        ones ``sac_targets()`` reads)."""
        if which not in _lib.SAC_NETS:
            raise ValueError(f"which must be one of {sorted(_lib.SAC_NETS)}")
        return self._export_net("ranenv_get_sac_net_weights", _lib.SAC_NETS[which])[0]

    def sac_log_ent_coef(self) -> torch.Tensor:
        """A copy of the binding's ``log_ent_coef`` float32 [1] as it is NOW (ranenv_get_sac_log_ent_coef); the coefficient the next
        step uses is ``exp`` of it in float64."""
        out = torch.empty((1,), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            self._check(self._lib.ranenv_get_sac_log_ent_coef(self._h, _ptr(out), self._stream()), "ranenv_get_sac_log_ent_coef")
        return out

    _SAC_STATE = {"actor": 0, "q1": 1, "q2": 2, "log_ent_coef": 3}

    def sac_state(self, which: str) -> Dict[str, torch.Tensor]:
        """Zero-copy views of the optimiser state of "actor", "q1", "q2" (packed layout) or "log_ent_coef" ([1]): Adam's "m" and "v"
        and "t", that tensor's step counter (ranenv_sac_state)."""
        if which not in self._SAC_STATE:
            raise ValueError(f"which must be one of {sorted(self._SAC_STATE)}")
        return self._opt_views("ranenv_sac_state", self._SAC_STATE[which])

    def head_episode_metrics(self) -> Dict[str, torch.Tensor]:
        """Zero-copy views of the episode sums of the two head rewards (columns: SchedTWC, SchedColORAN): ``running`` [B, 2]
        (current episode) and ``episode_log`` [B, slots, 2] (finished episodes, the rows of ``episode_metrics()``'s log; absent with
        0 slots).  They exist once both ``enable_metrics()`` and ``enable_heads()`` were called; after ``evaluate(n)`` the log's
        first n rows are the episodes it returned."""
        run, log = C.c_void_p(), C.c_void_p()
        slots = C.c_int32()
        self._check(self._lib.ranenv_get_head_metrics(self._h, C.byref(run), C.byref(log), C.byref(slots)), "ranenv_get_head_metrics")
        if not run.value:
            raise RanEnvError("head episode metrics need enable_metrics() and enable_heads()")
        out = {"running": torch.as_tensor(_DevArray(run.value, (self.B, 2), "f8", self), device=self.device)}
        if slots.value > 0 and log.value:
            out["episode_log"] = torch.as_tensor(_DevArray(log.value, (self.B, slots.value, 2), "f8", self), device=self.device)
        return out

    def policy_actions(self) -> Dict[str, Optional[torch.Tensor]]:
        """Zero-copy views of the last actions of the policy nets: ``scores`` float64 [B, S] (what the step read, in the
        sorted order of obs_inter) and ``intra`` uint8 [B, S] (by slice; None without an intra net)."""
        if getattr(self, "_policy_views", None) is None:
            sc, ic = C.c_void_p(), C.c_void_p()
            self._check(self._lib.ranenv_get_policy_actions(self._h, C.byref(sc), C.byref(ic)), "ranenv_get_policy_actions")
            self._policy_views = {
                "scores": torch.as_tensor(_DevArray(sc.value, (self.B, self.S), "f8", self), device=self.device),
                "intra": None if not ic.value else torch.as_tensor(_DevArray(ic.value, (self.B, self.S), "u1", self), device=self.device)}
        return self._policy_views

    _EP_DTYPE = [("scenario", "<i4"), ("se_len", "<i4"), ("se_base", "<i8"), ("se_offset", "<i4"), ("trf_len", "<i4"),
                 ("trf_base", "<i8"), ("trf_offset", "<i4"), ("reserved", "<i4")]

    def _episode_array(self, n, scenario, se_base, se_len, se_offset, trf_base, trf_len, trf_offset):
        eps = np.zeros(n, dtype=self._EP_DTYPE)
        assert eps.dtype.itemsize == C.sizeof(_lib.Episode)
        for k, v in (("scenario", scenario), ("se_len", se_len), ("se_base", se_base), ("se_offset", se_offset),
                     ("trf_len", trf_len), ("trf_base", trf_base), ("trf_offset", trf_offset)):
            eps[k] = np.broadcast_to(np.asarray(v), (n,))
        return eps

    def episode_descriptors(self) -> np.ndarray:
        """The per-env episode descriptors as they are on the device now (structured array; one small D2H)."""
        if not self._autoreset:
            return self.episodes
        raw = self.views()["episodes"].cpu().numpy()
        return np.ascontiguousarray(raw).view(self._EP_DTYPE).reshape(self.B)

    def set_traffic_generator(self, seed: int, env_id_base: int = 0, enable: bool = True):
        """Draw the offered traffic on the device -- Poisson(slice Mbps) * 1e6 bits per UE and TTI
        (traffics/mult_slice.py:24-32), Philox-4x32-10 keyed (seed; env_id_base + env, episode, step, UE) --
        instead of replaying the traffic pool.  ``enable=False`` goes back to the pool and keeps the last ``env_id_base``."""
        with torch.cuda.device(self.device):
            self._check(self._lib.ranenv_set_traffic_generator(self._h, 1 if enable else 0, int(seed) & (2 ** 64 - 1),
                                                               int(env_id_base), self._stream()), "ranenv_set_traffic_generator")
        # (disabling keeps the env id base: the policy noise and the random auto-reset draws stay keyed by it)
        if enable:
            self.traffic_seed, self.env_id_base = int(seed) & (2 ** 64 - 1), int(env_id_base)
        else:
            self.traffic_seed = None

    def poisson_tables(self):
        """Diagnostic: the traffic generator's inversion tables -> (cdf uint64 [NS, S, 256], guide uint8 [NS, S, 64])."""
        cdf = np.zeros((self.n_scenarios, self.S, 256), dtype=np.uint64)
        guide = np.zeros((self.n_scenarios, self.S, 64), dtype=np.uint8)
        with torch.cuda.device(self.device):
            self._check(self._lib.ranenv_get_poisson_tables(self._h, C.c_void_p(cdf.ctypes.data), C.c_void_p(guide.ctypes.data)),
                        "ranenv_get_poisson_tables")
        return cdf, guide

    def set_max_steps(self, max_steps=None):
        """Per-env episode length ([B] ints) or None for the constructor's max_steps everywhere."""
        if max_steps is None:
            self._check(self._lib.ranenv_set_max_steps(self._h, None, self._stream()), "ranenv_set_max_steps")
            self.max_steps_env = None
            return
        a = np.ascontiguousarray(np.broadcast_to(np.asarray(max_steps, dtype=np.int32), (self.B,)))
        with torch.cuda.device(self.device):
            self._check(self._lib.ranenv_set_max_steps(self._h, C.c_void_p(a.ctypes.data), self._stream()), "ranenv_set_max_steps")
        self.max_steps_env = a.copy()

    def set_episode_table(self, scenario, se_base=0, se_len=1, se_offset=0, trf_base=0, trf_len=1, trf_offset=0,
                          first_episode: int = 0):
        """Descriptor of every episode number in [first_episode, first_episode + len(scenario)): what the plugins'
        choose_episode resolves per episode (associations/mult_slice.py:444-452, channels/quadriga.py:78-87)."""
        n = len(np.atleast_1d(scenario))
        tab = self._episode_array(n, scenario, se_base, se_len, se_offset, trf_base, trf_len, trf_offset)
        with torch.cuda.device(self.device):
            self._check(self._lib.ranenv_set_episode_table(self._h, C.c_void_p(tab.ctypes.data), int(first_episode), n,
                                                           self._stream()), "ranenv_set_episode_table")
        self.episode_table, self.episode_table_first = tab, int(first_episode)

    def enable_autoreset(self, initial_episode: int, max_episode: int, random_episodes: bool = False, seed: int = 0,
                         episode_numbers=None, shortcut: bool = True):
        """After every step, envs that reported ``done`` move to their next episode on the device (sequential, or
        random in [initial, max) like enable_random_episodes, simu.py:361,377) and are reset, without a host sync.
        ``episode_numbers`` [B]: the episode every env plays now (its descriptor is installed here).  The terminal
        observation of those envs is kept in ``term_obs_inter`` / ``term_obs_intra`` (/ ``term_head_obs``).
        ``shortcut`` (library option ``autoreset_shortcut``): this class calls ranenv_autoreset right behind the step, inside
        ``step()`` / ``step_async()``, with its own ``done`` buffer -- nobody can have touched the flags in between -- so the
        library may follow the step counters on the host and enqueue nothing at a TTI at which no episode ended.  Pass
        ``False`` if you write to ``views()["step_number"]`` (the views are cached here: the library cannot see later writes)."""
        ep = None
        if episode_numbers is not None:
            ep = np.ascontiguousarray(np.broadcast_to(np.asarray(episode_numbers, dtype=np.int32), (self.B,)))
            rows = ep - self.episode_table_first
            if rows.min() < 0 or rows.max() >= len(self.episode_table):
                raise RanEnvError("episode_numbers outside the episode table")
            t = self.episode_table[rows]
            self.set_episodes(scenario=t["scenario"], se_base=t["se_base"], se_len=t["se_len"], se_offset=t["se_offset"],
                              trf_base=t["trf_base"], trf_len=t["trf_len"], trf_offset=t["trf_offset"])
        with torch.cuda.device(self.device):
            self._check(self._lib.ranenv_set_autoreset(self._h, 1, int(initial_episode), int(max_episode),
                                                       1 if random_episodes else 0, int(seed) & (2 ** 64 - 1),
                                                       None if ep is None else C.c_void_p(ep.ctypes.data), self._stream()),
                        "ranenv_set_autoreset")
        self.set_option("autoreset_shortcut", 1 if shortcut else 0)
        self.term_obs_inter = torch.zeros_like(self.obs_inter)
        self.term_obs_intra = torch.zeros_like(self.obs_intra)
        if getattr(self, "head_obs", None) is not None:
            self.term_head_obs = torch.zeros_like(self.head_obs)
        self._autoreset = True

    def disable_autoreset(self):
        self._check(self._lib.ranenv_set_autoreset(self._h, 0, 0, 0, 0, 0, None, self._stream()), "ranenv_set_autoreset")
        self._autoreset = False

    def _after_step(self):
        if self._recorder is not None:
            self._recorder.on_step(self.done)
        if self._autoreset:
            st = self._lib.ranenv_autoreset(self._h, _ptr(self.done), _ptr(self.obs_inter), _ptr(self.obs_intra),
                                            _ptr(self.term_obs_inter), _ptr(self.term_obs_intra), _ptr(self.term_head_obs),
                                            self._stream())
            if st != 0:
                self._check(st, "ranenv_autoreset")

    def record(self, envs, root_path: str = ".", simu_name: str = "mult_slice", agent_name: str = "agent",
               episode_numbers=None, marl: bool = True):
        """Record the listed envs into a device trace (``bind_trace``) and, under ``step()``, write
        ``hist/{simu_name}/{agent_name}/ep_{n}.npz`` (the 16 keys of results/gen_results.py:88-108) at the TTI one of them reports
        ``done``.  ``record(None)`` stops recording and unbinds that trace.  Returns the recorder (``.written`` lists the files)."""
        if self._recorder is not None:
            self._recorder = None
            self.unbind_trace()
        if envs is None:
            return None
        from .history import HistoryRecorder
        if self.tables is None or self.episodes is None:
            raise RanEnvError("record() needs load_scenarios + set_episodes first")
        if self._trace is not None:
            raise RanEnvError("record() binds a trace of its own and a handle holds one: unbind_trace() first")
        self._recorder = HistoryRecorder(self, envs, root_path, simu_name, agent_name, episode_numbers, marl)
        return self._recorder

    def bind_trace(self, envs, capacity: int, se: bool = True, guard_rows: int = 0):
        """Record the per-TTI history of the listed envs ON THE DEVICE, behind every step of whatever call steps them --
        ``rollout()``, ``evaluate()``, ``collect()``, ``collect_head()``, ``collect_replay()``, ``step()``, ``step_async()``, with or
        without partitions -- into a ring of ``capacity`` rows per env (ranenv_bind_trace, include/ranenv.h): what a history file
        holds of a TTI, and per row the step index, episode number, scenario and ``done``.  A full ring stops recording and counts
        the rows it lost.  ``se=False`` leaves the SE tile (4 R U of a row's bytes) out; such a trace cannot ``write()`` history
        files.  ``record()`` binds one of its own: not both at a time.  ``guard_rows``: rows allocated behind the
        ring and filled with 0xA5 bytes that the library is not told about (``trace.guard``: a check that nothing writes there).
        Returns the DeviceTrace (history.py: ``.buffers``, ``.counts()``, ``.episodes()``, ``.write()``).  While bound, a rollout runs
        one TTI per launch and no persistent launch, as with slice metrics on."""
        from .history import DeviceTrace
        if self.tables is None:
            raise RanEnvError("bind_trace() needs load_scenarios first")
        if self._recorder is not None:
            raise RanEnvError("bind_trace(): record() holds the handle's trace: record(None) first")
        envs = [int(e) for e in envs]
        n, cap, guard_rows = len(envs), int(capacity), int(guard_rows)
        dims = {"U": (self.U,), "RU": (self.R, self.U), "P": (self.S + 1,), "S": (self.S,), "I": (10 * self.S,), "SW": (self.S, self.W),
                "": ()}
        tr = _lib.Trace()
        tr.n_envs, tr.capacity = n, cap
        ids = np.ascontiguousarray(envs, dtype=np.int32)
        tr.envs = ids.ctypes.data
        full = {}
        if n >= 1 and cap >= 1 and guard_rows >= 0:        # (else: nothing to allocate; the library words the refusal)
            for name, ts, shp in _lib.TRACE_FIELDS:
                if name == "se" and not se:
                    continue
                full[name] = torch.zeros((cap + guard_rows, n) + dims[shp], dtype=_TORCH_DT[ts], device=self.device)
                if guard_rows:
                    full[name][cap:].view(torch.uint8).fill_(0xA5)
                setattr(tr, name, full[name].data_ptr())
        with torch.cuda.device(self.device):
            self._check(self._lib.ranenv_bind_trace(self._h, C.byref(tr), self._stream()), "ranenv_bind_trace")
        self._keep["trace"] = full
        cnt, lost = C.c_void_p(), C.c_void_p()
        self._check(self._lib.ranenv_get_trace_counts(self._h, C.byref(cnt), C.byref(lost)), "ranenv_get_trace_counts")
        d_cnt = torch.as_tensor(_DevArray(cnt.value, (n,), "i4", self), device=self.device)
        d_lost = torch.as_tensor(_DevArray(lost.value, (n,), "i4", self), device=self.device)

        def reset(columns=None):
            if columns is None:
                self._check(self._lib.ranenv_reset_trace(self._h, self._stream()), "ranenv_reset_trace")
            else:                                          # the library's counters, written in stream order
                cols = torch.as_tensor(list(columns), dtype=torch.int64, device=self.device)
                d_cnt.index_fill_(0, cols, 0)
                d_lost.index_fill_(0, cols, 0)

        self._trace = DeviceTrace(envs, cap, {k: b[:cap] for k, b in full.items()}, lambda: (d_cnt.cpu().numpy(), d_lost.cpu().numpy()),
                                  self.tables, self.R, self.Us, guard={k: b[cap:] for k, b in full.items()}, reset_fn=reset)
        return self._trace

    def unbind_trace(self) -> None:
        """Stop recording (ranenv_bind_trace with NULL).  The DeviceTrace handed out keeps its buffers and can still be read and
        written, its counters included, until the next ``bind_trace``."""
        if self._recorder is not None:
            raise RanEnvError("unbind_trace(): the bound trace is record()'s: record(None) stops recording and unbinds it")
        self._check(self._lib.ranenv_bind_trace(self._h, None, self._stream()), "ranenv_bind_trace")
        self._trace = None
        self._keep.pop("trace", None)

    # ------------------------------------------------------------------------------------------
    def _obs(self):
        return self._obs_dict

    def reset(self, env_mask=None, se_tiles=None):
        """CommunicationEnv.reset for the masked envs (all when None); returns the formatted obs."""
        m = self._dev(env_mask, torch.uint8, (self.B,), "env_mask")
        se = self._dev(se_tiles, torch.float32, (self.B, self.R, self.U), "se_tiles")
        with torch.cuda.device(self.device):
            self._check(self._lib.ranenv_reset(self._h, _ptr(m), _ptr(se), _ptr(self.obs_inter),
                                                _ptr(self.obs_intra), _ptr(self.reward), self._stream()),
                        "ranenv_reset")
        self._keep["last_inputs"] = (m, se)
        if self._recorder is not None:
            self._recorder.on_reset(m)
        return self._obs()

    def step(self, inter_scores=None, intra_choice=None, traffic_bits=None, se_tiles=None):
        """One TTI for all envs.  Returns (obs, reward [B,S+1] float64, done [B] uint8)."""
        if inter_scores is None and intra_choice is None and traffic_bits is None and se_tiles is None:
            # device policy + pools: nothing to marshal, just enqueue the launch
            st = self._step_fn(self._h, None, None, None, None, *self._p_out,
                               C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream))
            if st != 0:
                self._check(st, "ranenv_step")
            if self._recorder is not None or self._autoreset:
                self._after_step()
            return self._obs(), self.reward, self.done
        sc = self._dev(inter_scores, torch.float64, (self.B, self.S), "inter_scores")
        ic = self._dev(intra_choice, torch.uint8, (self.B, self.S), "intra_choice")
        tr = self._dev(traffic_bits, torch.float64, (self.B, self.U), "traffic_bits")
        se = self._dev(se_tiles, torch.float32, (self.B, self.R, self.U), "se_tiles")
        with torch.cuda.device(self.device):
            self._check(self._lib.ranenv_step(self._h, _ptr(sc), _ptr(ic), _ptr(tr), _ptr(se), _ptr(self.obs_inter),
                                               _ptr(self.obs_intra), _ptr(self.reward), _ptr(self.done),
                                               self._stream()), "ranenv_step")
        self._keep["last_inputs"] = (sc, ic, tr, se)
        if self._recorder is not None or self._autoreset:
            self._after_step()
        return self._obs(), self.reward, self.done

    # -- a learner in the loop: ranges of the batch stepped alternately on their own streams -------------------------
    def set_ranges(self, n_ranges: int = 2):
        """Cut the batch into ``n_ranges`` contiguous ranges (the batch partitions of ``set_partitions``), each with its
        own HIP stream, for ``step_async`` / ``step_wait``: while the policy consumes one range's observations, the other
        ranges' TTIs occupy the GPU (the reference trains through env.step with 10 concurrent env runners,
        simu.py:555-566, agents/ray_agent.py:296-300).  Returns the ranges [(lo, hi), ...]."""
        self.set_partitions(n_ranges)
        lo, n = C.c_int32(), C.c_int32()
        self._ranges = []
        for k in range(n_ranges):
            self._check(self._lib.ranenv_get_partition(self._h, k, C.byref(lo), C.byref(n)), "ranenv_get_partition")
            self._ranges.append((lo.value, lo.value + n.value))
        self._range_out = [({"obs_inter": self.obs_inter[lo:hi], "obs_intra": self.obs_intra[lo:hi]}, self.reward[lo:hi],
                            self.done[lo:hi]) for lo, hi in self._ranges]
        self._range_streams = {}
        return list(self._ranges)

    def range_stream(self, k: int) -> "torch.cuda.Stream":
        """Range ``k``'s own HIP stream as a torch stream.  A learner that runs range k's policy inside
        ``with torch.cuda.stream(env.range_stream(k)):`` and calls ``step_wait(k)`` / ``step_async(k, ...)`` there makes
        range k one in-order chain TTI -> policy -> TTI on one hardware queue: no event crosses between queues (each such
        hop costs ~15 us on this GPU), and the ranges' chains overlap on the GPU like concurrent env runners."""
        if self._ranges is None:
            raise RanEnvError("range_stream needs set_ranges() first")
        if k not in self._range_streams:
            p = C.c_void_p()
            self._check(self._lib.ranenv_get_part_stream(self._h, int(k), C.byref(p)), "ranenv_get_part_stream")
            self._range_streams[k] = torch.cuda.ExternalStream(p.value, device=self.device)
        return self._range_streams[k]

    def step_async(self, k: int, inter_scores=None, intra_choice=None, traffic_bits=None, se_tiles=None):
        """Enqueue one TTI of range ``k`` on that range's stream, ordered behind what the caller's current stream holds
        now (the kernels that produced the scores).  The arguments are whole-batch tensors ([B, ...], already on the
        device: nothing is converted here); only range k's rows are read and written, and the caller must leave those
        rows alone until ``step_wait(k)``.  Returns at once (one library call: ranenv_step_part; with ``enable_autoreset``
        a second one, ranenv_autoreset_part: finished envs of the range restart behind the step, ``done`` / ``reward`` keep
        the terminal transition, ``term_obs_*`` the terminal observation)."""
        if self._ranges is None:
            raise RanEnvError("step_async needs set_ranges() first")
        if self._recorder is not None:
            raise RanEnvError("step_async does not run the history recorder: use step()")
        for name, x, dt in (("inter_scores", inter_scores, torch.float64), ("intra_choice", intra_choice, torch.uint8),
                            ("traffic_bits", traffic_bits, torch.float64), ("se_tiles", se_tiles, torch.float32)):
            if x is not None and not (x.dtype == dt and x.device == self.device and x.shape[0] == self.B and x.is_contiguous()):
                raise RanEnvError(f"step_async: {name} must be a contiguous {dt} tensor [B, ...] on {self.device}")
        cur = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        st = self._lib.ranenv_step_part(self._h, k, _ptr(inter_scores), _ptr(intra_choice), _ptr(traffic_bits), _ptr(se_tiles),
                                        *self._p_out, cur)
        if st != 0:
            self._check(st, "ranenv_step_part")
        if self._autoreset:       # the range's finished envs move on to their next episode behind the step, on the range's stream
            st = self._lib.ranenv_autoreset_part(self._h, k, _ptr(self.done), _ptr(self.obs_inter), _ptr(self.obs_intra),
                                                 _ptr(self.term_obs_inter), _ptr(self.term_obs_intra), _ptr(self.term_head_obs), cur)
            if st != 0:
                self._check(st, "ranenv_autoreset_part")
        # the inputs are read on the range's stream: they stay referenced here until the range's next launch (their
        # memory must not go back to the caching allocator meanwhile)
        self._keep[("async_inputs", k)] = (inter_scores, intra_choice, traffic_bits, se_tiles)

    def step_wait(self, k: int):
        """Order the caller's current stream behind range ``k``'s last ``step_async`` (no host sync) and return views of
        that range's rows: ({"obs_inter", "obs_intra"}, reward, done).  They are zero-copy views of buffers the range's NEXT
        step_async overwrites in place from a HIP kernel (autograd's version counters do not see it): clone whatever a
        graph or a replay buffer keeps beyond that call."""
        st = self._lib.ranenv_wait_part(self._h, k, C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream))
        if st != 0:
            self._check(st, "ranenv_wait_part")
        return self._range_out[k]

    def step_dense(self, sched_decision, traffic_bits=None, se_tiles=None):
        """One TTI with a caller-made dense sched_decision [B,U,R] (any agent's action_format)."""
        sd = self._dev(sched_decision, torch.uint8, (self.B, self.U, self.R), "sched_decision")
        tr = self._dev(traffic_bits, torch.float64, (self.B, self.U), "traffic_bits")
        se = self._dev(se_tiles, torch.float32, (self.B, self.R, self.U), "se_tiles")
        with torch.cuda.device(self.device):
            self._check(self._lib.ranenv_step_dense(self._h, _ptr(sd), _ptr(tr), _ptr(se), _ptr(self.obs_inter),
                                                     _ptr(self.obs_intra), _ptr(self.reward), _ptr(self.done),
                                                     self._stream()), "ranenv_step_dense")
        self._keep["last_inputs"] = (sd, tr, se)
        return self._obs(), self.reward, self.done

    # ------------------------------------------------------------------------------------------
    def enable_heads(self, slice_usecase=None):
        """Also compute the SchedTWC / SchedColORAN observation and rewards every TTI
        (agents/sched_twc.py:165-413, agents/sched_colran.py:348-419).

        ``self.head_obs``  float32 [B, 10*S]: per slice 3 requirement values, then the slice means of SE,
        served Mbps, effective Mbps, buffer occupancy, buffer latency, loss rate and the requested Mbps
        (metric-major, slices in index order); ``self.head_reward`` float64 [B, 2] = (SchedTWC, SchedColORAN).
        ``slice_usecase``: int [n_scenarios, S], bit 0 eMBB / bit 1 URLLC (scenario.slice_usecase_from_req).
        Their action is IBSched's with round-robin inside the slices: ``set_policy(POLICY_EXTERNAL, INTRA_RR)``.
        """
        self.head_obs = torch.zeros((self.B, 10 * self.S), dtype=torch.float32, device=self.device)
        self.head_reward = torch.zeros((self.B, 2), dtype=torch.float64, device=self.device)
        self._check(self._lib.ranenv_bind_head_outputs(self._h, _ptr(self.head_obs), _ptr(self.head_reward)),
                    "ranenv_bind_head_outputs")
        if self._autoreset:
            self.term_head_obs = torch.zeros_like(self.head_obs)
        if slice_usecase is not None:
            self.set_slice_usecase(slice_usecase)

    def set_slice_usecase(self, slice_usecase, first: int = 0):
        uc = np.ascontiguousarray(slice_usecase, dtype=np.int32).reshape(-1, self.S)
        with torch.cuda.device(self.device):
            self._check(self._lib.ranenv_set_slice_usecase(self._h, int(first), uc.shape[0], C.c_void_p(uc.ctypes.data),
                                                           self._stream()), "ranenv_set_slice_usecase")

    # ------------------------------------------------------------------------------------------
    def views(self) -> Dict[str, torch.Tensor]:
        """Zero-copy torch views of the handle's raw-observation and state arrays."""
        if self._views is None:
            v = _lib.Views()
            self._check(self._lib.ranenv_get_views(self._h, C.byref(v)), "ranenv_get_views")
            dims = {"B": self.B, "U": self.U, "S": self.S, "K": self.Us, "E": C.sizeof(_lib.Episode) // 4}
            out = {}
            for name, ts, shp in _lib.VIEW_FIELDS:
                shape = tuple(dims[c] for c in shp)
                arr = _DevArray(getattr(v, name), shape, ts, self)
                out[name] = torch.as_tensor(arr, device=self.device)
                assert out[name].dtype == _TORCH_DT[ts]
            self._views = out
        return self._views

    def raw_observation(self) -> Dict[str, torch.Tensor]:
        """The reference's raw-observation metric fields (agents/ib_sched.py:78-181), batched."""
        v = self.views()
        if self.tables is None or self.episodes is None:
            raise RanEnvError("raw_observation needs load_scenarios + set_episodes")
        scen = v["episodes"][:, 0].to(torch.int64)           # as on the device: auto-reset may have moved on
        max_pkts = torch.as_tensor(self.tables.ue_max_pkts, device=self.device)[scen].to(torch.float64)
        q = v["queue_pkts"].to(torch.float64)
        lat = torch.where(q > 0, v["queue_age_sum"].to(torch.float64) / q.clamp(min=1), torch.zeros_like(q))
        return {
            "pkt_incoming": v["pkt_incoming"].to(torch.float64),
            "pkt_throughputs": v["pkt_throughputs"].to(torch.float64),
            "pkt_effective_thr": v["pkt_effective_thr"].to(torch.float64),
            "dropped_pkts": v["dropped_pkts"].to(torch.float64),
            "buffer_occupancies": q / max_pkts,
            "buffer_latencies": lat,
        }

    def profile_begin(self):
        """Time every launch of the step kernel from here on (the dispatch's own start / stop timestamps)."""
        self._check(self._lib.ranenv_profile_begin(self._h), "ranenv_profile_begin")

    def profile_end(self) -> Dict[str, float]:
        """Average duration in ms of the step-kernel launches since profile_begin: {'step', 'n_launches', 'n_ttis'}
        (inside rollout() a launch may cover several TTIs: n_ttis / n_launches of them on average; n_env_ttis = envs x TTIs
        summed over the launches)."""
        ms, n, nt, ne = C.c_double(), C.c_int32(), C.c_int64(), C.c_int64()
        self._check(self._lib.ranenv_profile_end(self._h, C.byref(ms), C.byref(n)), "ranenv_profile_end")
        self._check(self._lib.ranenv_profile_work(self._h, C.byref(nt), C.byref(ne)), "ranenv_profile_work")
        return {"step": ms.value, "n_launches": n.value, "n_ttis": nt.value, "n_env_ttis": ne.value}

    def set_partitions(self, n_parts: int):
        """Step the batch as ``n_parts`` contiguous ranges of envs, each by its own launch on its own stream
        (ranenv_set_partitions): one range's launch ramp and tail then run under the others' steady state."""
        with torch.cuda.device(self.device):
            self._check(self._lib.ranenv_set_partitions(self._h, int(n_parts)), "ranenv_set_partitions")
        self.n_parts = int(n_parts)

    def rollout(self, n_steps: int):
        """``n_steps`` TTIs under the device policy enqueued in one call (MARR / MAPF / policy-network evaluation runs): the launches of
        ``n_steps`` calls of ``step()``, joined with the current stream only before the first and after the last TTI
        -- except that one launch takes its envs through up to n_steps / 4 (at most 10) TTIs where nothing has to happen in
        between (no head kernel; with auto-reset: up to the TTI at which an episode of the batch ends).  Same results bit
        for bit.  Returns the last TTI's (obs, reward, done)."""
        if self._recorder is not None:
            raise RanEnvError("rollout() does not return between TTIs: the recorder needs step()")
        st = self._lib.ranenv_rollout(self._h, int(n_steps), *self._p_out,
                                      C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream))
        if st != 0:
            self._check(st, "ranenv_rollout")
        return self._obs(), self.reward, self.done

    METRIC_NAMES = ("ttis", "reward", "violations", "priority_violations", "distance", "priority_distance",
                    "pkts_sent", "pkts_dropped")

    def enable_metrics(self, episode_slots: int = 0) -> None:
        """Per-env running sums over the TTIs of the current episode, kept by the step kernel (include/ranenv.h:
        TTIs, inter-slice reward, slices in violation and distance to fulfilment for all / priority slices -- the
        quantities results/gen_results.py:874-1022 derives from the history files -- and packets sent / dropped).
        With auto-reset a finished episode's sums are appended to the env's log of ``episode_slots`` rows."""
        self._check(self._lib.ranenv_enable_metrics(self._h, int(episode_slots), self._stream()), "ranenv_enable_metrics")
        self._metric_views = None
        self._slice_metric_views = None

    def disable_metrics(self) -> None:
        """Switches the episode metrics off, the per-slice ones with them."""
        self._check(self._lib.ranenv_enable_metrics(self._h, -1, self._stream()), "ranenv_enable_metrics")
        self._slice_metrics_on = False

    SLICE_METRIC_NAMES = ("active_ttis", "violations", "viol_throughput", "viol_reliability", "viol_latency", "distance",
                          "pkts_incoming", "pkts_capacity", "pkts_sent", "pkts_dropped")

    def enable_slice_metrics(self) -> None:
        """Per-(env, slice) running sums over the TTIs of the current episode, kept by a small kernel behind every step
        (include/ranenv.h "Per-slice episode metrics": the per-slice quantities of results/gen_results.py:874-970, :791-809,
        :1007-1018; columns as SLICE_METRIC_NAMES, slices in index order).  Needs enable_metrics() first: the episode slots
        are its.  While on, rollout() runs one TTI per launch."""
        self._check(self._lib.ranenv_enable_slice_metrics(self._h, 1, self._stream()), "ranenv_enable_slice_metrics")
        self._slice_metric_views = None
        self._slice_metrics_on = True

    def disable_slice_metrics(self) -> None:
        self._check(self._lib.ranenv_enable_slice_metrics(self._h, 0, self._stream()), "ranenv_enable_slice_metrics")
        self._slice_metrics_on = False

    def slice_episode_metrics(self) -> Dict[str, torch.Tensor]:
        """Zero-copy views: ``running`` [B, S, 10] (current episode), and with episode slots ``episode_log`` [B, slots, S, 10]
        (finished episodes, in order) and ``episode_scenario`` [B, slots] int32 (the scenario-pool row each logged episode
        was played on, -1 = empty slot); columns as SLICE_METRIC_NAMES."""
        if getattr(self, "_slice_metric_views", None) is None:
            run, log, scn = C.c_void_p(), C.c_void_p(), C.c_void_p()
            ncol = C.c_int32()
            self._check(self._lib.ranenv_get_slice_metrics(self._h, C.byref(run), C.byref(log), C.byref(scn), C.byref(ncol)),
                        "ranenv_get_slice_metrics")
            K = ncol.value
            if K != len(self.SLICE_METRIC_NAMES):
                raise RanEnvError(f"the library keeps {K} per-slice columns, the binding names {len(self.SLICE_METRIC_NAMES)}")
            out = {"running": torch.as_tensor(_DevArray(run.value, (self.B, self.S, K), "f8", self), device=self.device)}
            if log.value:
                slots = int(self.episode_metrics()["episode_log"].shape[1])
                out["episode_log"] = torch.as_tensor(_DevArray(log.value, (self.B, slots, self.S, K), "f8", self), device=self.device)
                out["episode_scenario"] = torch.as_tensor(_DevArray(scn.value, (self.B, slots), "i4", self), device=self.device)
            self._slice_metric_views = out
        return self._slice_metric_views

    def episode_metrics(self) -> Dict[str, torch.Tensor]:
        """Zero-copy views: ``running`` [B, 8] (current episode), ``episode_log`` [B, slots, 8] (finished episodes, in
        order; absent with 0 slots), ``episodes_done`` [B]; columns as METRIC_NAMES."""
        if getattr(self, "_metric_views", None) is None:
            run, log, n = C.c_void_p(), C.c_void_p(), C.c_void_p()
            slots = C.c_int32()
            self._check(self._lib.ranenv_get_metrics(self._h, C.byref(run), C.byref(log), C.byref(n), C.byref(slots)), "ranenv_get_metrics")
            out = {"running": torch.as_tensor(_DevArray(run.value, (self.B, 8), "f8", self), device=self.device),
                   "episodes_done": torch.as_tensor(_DevArray(n.value, (self.B,), "i4", self), device=self.device)}
            if slots.value > 0:
                out["episode_log"] = torch.as_tensor(_DevArray(log.value, (self.B, slots.value, 8), "f8", self), device=self.device)
            self._metric_views = out
        return self._metric_views

    def evaluate(self, n_episodes: int, max_steps=None, per_slice: bool = False) -> Dict[str, np.ndarray]:
        """The reference's test loop for its baseline agents (simu.py:547-566 over ``max_episode - initial_episode``
        episodes; the numbers results/gen_results.py:874-1022 turns into the paper's violation / distance figures), for
        the whole batch on the device: reset, then one rollout long enough for every env to finish ``n_episodes``
        episodes under the device policy, episode ends handled by auto-reset.  Needs enable_autoreset(...) and
        enable_metrics(slots >= n_episodes).  Returns {metric: float64 [B, n_episodes]} with the names of METRIC_NAMES;
        row b holds env b's episodes in the order it played them (from the episode number given to enable_autoreset).
        ``per_slice`` (needs enable_slice_metrics()): the result gains ``"slice"``, float64 [B, n_episodes, S, 10] with the
        columns of SLICE_METRIC_NAMES, and ``"scenario"``, int32 [B, n_episodes]: the scenario-pool row of every episode,
        which says what slice type each slice index was (scenario.slice_type_report aggregates by type)."""
        if not self._autoreset:
            raise RanEnvError("evaluate() needs enable_autoreset(): it runs through episode ends on the device")
        if per_slice and not getattr(self, "_slice_metrics_on", False):
            raise RanEnvError("evaluate(per_slice=True) needs enable_slice_metrics()")
        m = self.episode_metrics()
        if "episode_log" not in m or m["episode_log"].shape[1] < n_episodes:
            raise RanEnvError(f"evaluate({n_episodes}) needs enable_metrics(episode_slots >= {n_episodes})")
        if max_steps is not None:
            self.set_max_steps(max_steps)
        me = getattr(self, "max_steps_env", None)
        longest = int(self.max_steps) if me is None else int(me.max())
        self.enable_metrics(m["episode_log"].shape[1])      # zero the sums and the log (the per-slice ones too while they are on)
        m = self.episode_metrics()
        sm = self.slice_episode_metrics() if per_slice else None
        self.reset()
        self.rollout(n_episodes * longest)
        torch.cuda.synchronize(self.device)
        done = m["episodes_done"].cpu().numpy()
        if done.min() < n_episodes:
            raise RanEnvError(f"an env finished only {int(done.min())} of {n_episodes} episodes: per-env max_steps longer than assumed")
        log = m["episode_log"][:, :n_episodes].cpu().numpy()
        out = {name: log[:, :, k].copy() for k, name in enumerate(self.METRIC_NAMES)}
        if per_slice:
            out["slice"] = sm["episode_log"][:, :n_episodes].cpu().numpy()
            out["scenario"] = sm["episode_scenario"][:, :n_episodes].cpu().numpy()
        return out

    def set_option(self, key: str, value: int) -> None:
        """A tuning / debug knob of the launch schedule; the keys are the table "Options" in include/ranenv.h.  None of them
        changes a result."""
        self._check(self._lib.ranenv_set_option(self._h, key.encode(), int(value)), f"ranenv_set_option({key})")

    def get_option(self, key: str) -> int:
        v = C.c_int64()
        self._check(self._lib.ranenv_get_option(self._h, key.encode(), C.byref(v)), f"ranenv_get_option({key})")
        return int(v.value)

    STEP_BUILDS = ("lean", "small", "gather", "tiny1", "mixed", "packed", "persist", "persist_tiny")

    def step_launches(self) -> Dict[str, int]:
        """Which build of the step kernel this handle's step launches ran: per build in STEP_BUILDS the launches enqueued since
        create under "<build>", and those of several TTIs under "<build>_many" (the read-only options "step_launches_*")."""
        out = {}
        for b in self.STEP_BUILDS:
            out[b] = self.get_option("step_launches_" + b)
            out[b + "_many"] = self.get_option("step_launches_" + b + "_many")
        return out

    def launch_info(self):
        g, b, l = C.c_int32(), C.c_int32(), C.c_int32()
        self._check(self._lib.ranenv_launch_info(self._h, C.byref(g), C.byref(b), C.byref(l)), "ranenv_launch_info")
        return {"grid": g.value, "block": b.value, "lds_bytes": l.value}

    def algorithmic_bytes_per_env_step(self, se_mode: Optional[str] = None) -> int:
        """4*U*R + 180*U + S*(85 + 8*Us) + 4 for the streaming step.  The gather mode replaces the
        tile term 4*U*R by what it reads of a tile: the R allocated elements (every RB belongs to one UE) and the per-UE
        mean row of the sidecar, 4*R + 8*U."""
        rest = 180 * self.U + self.S * (85 + 8 * self.Us) + 4
        if (se_mode or self.se_mode) == "gather":
            return 4 * self.R + 8 * self.U + rest
        return 4 * self.U * self.R + rest
