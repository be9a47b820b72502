"""Trainer-facing views of BatchedRanEnv.

* ``HeadVecEnv``: the single-agent, vectorised environment the reference's SB3 agents train on
  (``PPO("MlpPolicy", env)``, agents/sched_twc.py:112-118) -- observation and reward of SchedTWC or
  SchedColORAN from the head kernel, action = inter-slice scores with round-robin inside the slices
  (agents/sched_twc.py:415-422).  It follows the ``stable_baselines3.common.vec_env.VecEnv`` protocol
  (``num_envs``, ``reset``, ``step_async`` / ``step_wait`` / ``step``, auto-reset with
  ``infos[i]["terminal_observation"]``) and subclasses it when stable-baselines3 is importable.
* ``InterVecEnv``: the same protocol for the reference's IBSchedSB3 (agents/sb3_sched.py, agents/sb3_pf_sched.py), whose SB3 agent
  sees IBSched's own ``player_0`` observation and reward: ``obs_inter``, ``reward[:, 0]``, round-robin or proportional fair inside
  the slices.  The host-paced view of ``set_head_policy_network(observation="inter")``.
* ``marl_obs_dict`` / ``marl_reward_dict``: one env of the batch in the dict layout RLlib's policies
  of the reference consume (``player_0`` = inter-slice agent, ``player_{s+1}`` = intra-slice agents,
  agents/ib_sched.py:160-200, simu.py:559-566).
* ``head_policy_actions`` / ``head_policy_logp`` / ``sb3_ppo_layers`` / ``sb3_sac_actor_layers``: trained SchedTWC / SchedColORAN
  policies on the device (``BatchedRanEnv.set_head_policy_network``): the normative restatement and the SB3 state-dict readers.
"""
from __future__ import annotations

from typing import Dict, List, Optional

import numpy as np
import torch

from ._lib import INTRA_PF, INTRA_RR, POLICY_EXTERNAL
from .batched_env import BatchedRanEnv

try:  # optional: real base class and spaces when the trainer stack is installed
    from stable_baselines3.common.vec_env import VecEnv as _VecEnvBase   # type: ignore
except Exception:  # noqa: BLE001
    _VecEnvBase = object
try:
    from gymnasium import spaces as _spaces                             # type: ignore
except Exception:  # noqa: BLE001
    _spaces = None


class _Box:
    """Stand-in for gymnasium.spaces.Box when gymnasium is absent (shape / bounds / dtype holder)."""

    def __init__(self, low, high, shape, dtype):
        self.low, self.high, self.shape, self.dtype = low, high, tuple(shape), dtype


class _Discrete:
    """Stand-in for gymnasium.spaces.Discrete when gymnasium is absent."""

    def __init__(self, n):
        self.n = int(n)


class _Dict:
    """Stand-in for gymnasium.spaces.Dict when gymnasium is absent."""

    def __init__(self, spaces):
        self.spaces = dict(spaces)

    def __getitem__(self, key):
        return self.spaces[key]


def _box(low, high, shape, dtype):
    if _spaces is not None:
        return _spaces.Box(low=low, high=high, shape=tuple(shape), dtype=dtype)
    return _Box(low, high, shape, dtype)


def _discrete(n):
    return _spaces.Discrete(n) if _spaces is not None else _Discrete(n)


def _dict(spaces):
    return _spaces.Dict(spaces) if _spaces is not None else _Dict(spaces)


def describe_space(sp) -> dict:
    """A space (gymnasium's or the stand-ins above) as plain data: nested dicts of {"shape", "low", "high", "dtype"} /
    {"discrete": n}."""
    if hasattr(sp, "spaces"):
        return {k: describe_space(v) for k, v in sp.spaces.items()}
    if hasattr(sp, "n"):
        return {"discrete": int(sp.n)}
    return {"shape": list(sp.shape), "low": float(np.min(sp.low)), "high": float(np.max(sp.high)), "dtype": np.dtype(sp.dtype).name}


class _SingleAgentVecEnv(_VecEnvBase):
    """The VecEnv protocol of HeadVecEnv and InterVecEnv: B environments as one vector env for a single-agent trainer whose action is
    the inter-slice scores under a fixed intra-slice scheduler.  A subclass says which of the env's buffers are the agent's
    observation, its reward column and its terminal observation (``_observation`` / ``_reward_column`` / ``_terminal``)."""

    def _open(self, env: BatchedRanEnv, fixed_intra: int, observation_space, action_space):
        self.env = env
        env.set_policy(POLICY_EXTERNAL, fixed_intra)
        self.num_envs = env.B
        self.observation_space, self.action_space = observation_space, action_space
        if _VecEnvBase is not object:
            _VecEnvBase.__init__(self, self.num_envs, self.observation_space, self.action_space)
        self._intra = torch.zeros((env.B, env.S), dtype=torch.uint8, device=env.device)
        self._actions: Optional[torch.Tensor] = None

    # -- VecEnv protocol ------------------------------------------------------------------------
    def enable_device_autoreset(self, initial_episode: int, max_episode: int, random_episodes: bool = False, seed: int = 0,
                                episode_numbers=None):
        """Finished envs move to their next episode and are reset on the device (BatchedRanEnv.enable_autoreset;
        the env needs an episode table): ``step_wait`` then costs one device-to-host copy per step."""
        self.env.enable_autoreset(initial_episode, max_episode, random_episodes, seed, episode_numbers)

    def reset(self):
        self.env.reset()
        return self._observation().cpu().numpy()

    def step_async(self, actions):
        a = torch.as_tensor(np.asarray(actions), dtype=torch.float64, device=self.env.device)
        if tuple(a.shape) != (self.env.B, self.env.S):
            raise ValueError(f"actions must be [{self.env.B}, {self.env.S}]")
        self._actions = a.clamp(-1.0, 1.0)

    def step_wait(self):
        if self._actions is None:
            raise RuntimeError("step_async was not called")
        env = self.env
        _, _, done = env.step(self._actions, self._intra)
        self._actions = None
        infos: List[Dict] = [{} for _ in range(self.num_envs)]
        head_obs = self._observation()
        if env._autoreset:
            # one packed D2H: [observation (already the next episode's first one where done) | reward | done]
            n = head_obs.shape[1]
            packed = torch.cat([head_obs.to(torch.float64), self._reward_column()[:, None],
                                done.to(torch.float64)[:, None]], dim=1).cpu().numpy()
            obs, rew, dones = packed[:, :n].astype(np.float32), packed[:, n].astype(np.float32), packed[:, n + 1] != 0
            if dones.any():                                     # rare (once per episode and env): fetch the terminal rows
                idx = np.nonzero(dones)[0]
                term = self._terminal()[torch.as_tensor(idx, device=env.device)].cpu().numpy()
                for j, i in enumerate(idx):
                    infos[i]["terminal_observation"] = term[j]
                    infos[i]["TimeLimit.truncated"] = False
            return obs, rew, dones, infos
        obs = head_obs.cpu().numpy()
        rew = self._reward_column().cpu().numpy().astype(np.float32)
        dones = done.cpu().numpy().astype(bool)
        if dones.any():                                         # auto-reset from the host, as DummyVecEnv does
            for i in np.nonzero(dones)[0]:
                infos[i]["terminal_observation"] = obs[i].copy()
                infos[i]["TimeLimit.truncated"] = False
            env.reset(env_mask=dones.astype(np.uint8))
            obs[dones] = self._observation().cpu().numpy()[dones]
        return obs, rew, dones, infos

    def step(self, actions):
        self.step_async(actions)
        return self.step_wait()

    def close(self):
        self.env.close()

    # the rest of the VecEnv interface: nothing to delegate to (the envs live on the GPU)
    def get_attr(self, attr_name, indices=None):
        return [getattr(self.env, attr_name)] * self.num_envs

    def set_attr(self, attr_name, value, indices=None):
        setattr(self.env, attr_name, value)

    def env_method(self, method_name, *args, indices=None, **kwargs):
        return [getattr(self.env, method_name)(*args, **kwargs)] * self.num_envs

    def env_is_wrapped(self, wrapper_class, indices=None):
        return [False] * self.num_envs

    def seed(self, seed=None):
        return [None] * self.num_envs


class HeadVecEnv(_SingleAgentVecEnv):
    """B environments as one vector env for a single-agent trainer.

    ``reward``: "twc" (SchedTWC.calculate_reward) or "colran" (SchedColORAN.calculate_reward).
    ``slice_usecase``: [n_scenarios, S] eMBB / URLLC bits, needed by the "colran" reward
    (scenario.slice_usecase_from_req).  The env must already have scenarios, pools and episodes set.
    """

    def __init__(self, env: BatchedRanEnv, reward: str = "twc", slice_usecase=None):
        if reward not in ("twc", "colran"):
            raise ValueError("reward must be 'twc' or 'colran'")
        self._col = 0 if reward == "twc" else 1
        env.enable_heads(slice_usecase)
        S = env.S
        self._open(env, INTRA_RR, _box(-np.inf, np.inf, (10 * S,), np.float32),      # sched_twc.py:430-433
                   _box(-1.0, 1.0, (S,), np.float64))                                 # ib_sched.py:394-403

    def _observation(self):
        return self.env.head_obs

    def _reward_column(self):
        return self.env.head_reward[:, self._col]

    def _terminal(self):
        return self.env.term_head_obs


class InterVecEnv(_SingleAgentVecEnv):
    """The reference's IBSchedSB3 as a vector env (agents/sb3_sched.py; ``intra="pf"``: agents/sb3_pf_sched.py): the SB3 agent acts on
    IBSched's own player_0 terms -- observation ``obs_inter`` [10*S], slices in sorted positions, the action mask dropped
    (sb3_sched.py:159-162); reward ``reward[:, 0]`` (:164-167); action = inter-slice scores by sorted position with round-robin
    ("rr") or proportional fair ("pf") inside the slices (:169-177); terminal observations from ``term_obs_inter``.  Spaces as
    MarlBatchEnv declares them for player_0.  The env must already have scenarios, pools and episodes set; no ``enable_heads()``."""

    INTRA = {"rr": INTRA_RR, "pf": INTRA_PF}

    def __init__(self, env: BatchedRanEnv, intra: str = "rr"):
        if intra not in self.INTRA:
            raise ValueError("intra must be 'rr' or 'pf'")
        S = env.S
        self._open(env, self.INTRA[intra], _box(-1, np.inf, (S * 10,), np.float32),  # ib_sched.py:413-470, player_0
                   _box(-1, 1, (S,), np.float64))                                     # ib_sched.py:394-403

    def _observation(self):
        return self.env.obs_inter

    def _reward_column(self):
        return self.env.reward[:, 0]

    def _terminal(self):
        return self.env.term_obs_inter


def marl_obs_dict(env: BatchedRanEnv, b: int) -> Dict[str, Dict[str, np.ndarray]]:
    """Env ``b``'s last observation as IBSched.obs_space_format returns it (agents/ib_sched.py:160-200)."""
    v = env.views()
    out = {"player_0": {"observations": env.obs_inter[b].cpu().numpy().astype(np.float64),
                        "action_mask": v["mask_inter"][b].cpu().numpy().astype(np.int8)}}
    oa, ma = env.obs_intra[b].cpu().numpy(), v["mask_intra"][b].cpu().numpy()
    for s in range(env.S):
        out[f"player_{s + 1}"] = {"observations": oa[s].astype(np.float64), "action_mask": ma[s].astype(np.int8)}
    return out


def marl_reward_dict(env: BatchedRanEnv, b: int) -> Dict[str, float]:
    """Env ``b``'s last rewards as calculate_reward_no_mask returns them (agents/common.py:381-439)."""
    r = env.reward[b].cpu().numpy()
    return {f"player_{i}": float(r[i]) for i in range(env.S + 1)}


# --------------------------------------------------------------------------------------------
# the whole batch in the reference's RLlib layout, on the device
# --------------------------------------------------------------------------------------------
def sorted_action_mask(action_mask: torch.Tensor) -> torch.Tensor:
    """TorchActionMaskModel.forward's mask (agents/action_mask_model.py:46-50): the inter-slice observation lists the
    slices sorted by requested traffic, inactive ones first, so the mask handed to the action distribution has its
    last ``n_active`` entries set.  Batched: every row uses its own count (the reference takes row 0's for all)."""
    n = action_mask.to(torch.int64).sum(dim=-1, keepdim=True)
    S = action_mask.shape[-1]
    pos = torch.arange(S, device=action_mask.device).expand_as(action_mask)
    return (pos >= S - n).to(action_mask.dtype)


def masked_gaussian_params(mean: torch.Tensor, log_std: torch.Tensor, masks: torch.Tensor):
    """The inter-slice action distribution's parameters (agents/masked_action_distribution.py:30-36): std = exp(log_std);
    where the mask is 0 the mean is -1 and the std 1e-9, so an inactive slice always gets the score -1."""
    std = torch.exp(log_std)
    std = torch.where(masks == 0, torch.full_like(std, 1e-9), std)
    mean = torch.where(masks == 0, torch.full_like(mean, -1.0), mean)
    return mean, std


class MarlBatchEnv:
    """B environments in the multi-agent layout the reference trains RLlib policies on, as device tensors.

    Observation (IBSched.obs_space_format, agents/ib_sched.py:160-200; spaces :413-470):
        ``obs["player_0"]``     = {"observations": float32 [B, 10*S], "action_mask": int8 [B, S]}
        ``obs["player_{s+1}"]`` = {"observations": float32 [B, 2*Us+9], "action_mask": int8 [B, Us]}
    Action (IBSched.get_action_space :394-411): ``{"player_0": [B, S] scores in [-1, 1] (the masked diagonal Gaussian
    over S of masked_action_distribution.py), "player_{s+1}": [B] integers in {0, 1, 2} (Discrete(3): RR / PF / MT)}``.
    Reward: ``{"player_i": float64 [B]}``; terminated: ``{"player_i": bool [B], "__all__": bool [B]}`` (simu.py:559-564).
    All tensors are views of the env's buffers (zero copy); nothing here synchronises with the host.
    ``observation_space`` / ``action_space``: one env's spaces as IBSched.get_obs_space / get_action_space declare them
    (agents/ib_sched.py:394-470; gymnasium's classes when installed), with two differences: the per-slice observation has
    ``2 * max_ues_slice + 9`` entries (the reference hard-codes max_number_ues / max_number_slices UEs per slice) and
    observations are declared float32, which is what the device hands out.
    """

    def __init__(self, env: BatchedRanEnv):
        self.env = env
        env.set_policy(POLICY_EXTERNAL, 255)           # scores and schedulers come with every action
        self.players = [f"player_{i}" for i in range(env.S + 1)]
        self._intra = torch.zeros((env.B, env.S), dtype=torch.uint8, device=env.device)
        S, Us = env.S, env.Us
        self.action_space = _dict({p: (_box(-1, 1, (S,), np.float64) if i == 0 else _discrete(3))       # :394-411
                                   for i, p in enumerate(self.players)})
        self.observation_space = _dict({                                                                  # :413-470
            p: _dict({"observations": _box(-1, np.inf, (S * 10,) if i == 0 else (2 * Us + 9,), np.float32),
                      "action_mask": _box(0.0, 1.0, (S,) if i == 0 else (Us,), np.int8)})
            for i, p in enumerate(self.players)})

    def _obs(self):
        env, v = self.env, self.env.views()
        out = {"player_0": {"observations": env.obs_inter, "action_mask": v["mask_inter"]}}
        for s in range(env.S):
            out[f"player_{s + 1}"] = {"observations": env.obs_intra[:, s], "action_mask": v["mask_intra"][:, s]}
        return out

    def reset(self):
        self.env.reset()
        return self._obs(), {}

    def step(self, action: Dict[str, torch.Tensor]):
        env = self.env
        scores = action["player_0"].to(device=env.device, dtype=torch.float64)
        self._intra.copy_(torch.stack([action[f"player_{s + 1}"].to(env.device) for s in range(env.S)], dim=1))
        _, reward, done = env.step(scores, self._intra)
        rew = {p: reward[:, i] for i, p in enumerate(self.players)}
        d = done != 0
        term = {p: d for p in self.players}
        term["__all__"] = d
        trunc = {p: torch.zeros_like(d) for p in term}
        return self._obs(), rew, term, trunc, {}


# --------------------------------------------------------------------------------------------
# trained IBSched policies on the device (RANENV_POLICY_NETWORK): the normative restatement and the checkpoint reader
# --------------------------------------------------------------------------------------------
POLICY_TAG = 0x504F4C00          # counter word c3 of the policy's Philox draws: tag + slice (include/ranenv.h)


def philox4x32_10(c0, c1, c2, c3, k0: int, k1: int):
    """Philox-4x32-10 (Salmon, Moraes, Dror, Shaw, SC'11) on numpy arrays (broadcast): the generator of the device's
    policy noise.  Returns four uint64 arrays holding 32-bit words."""
    m32 = np.uint64(0xFFFFFFFF)
    c0, c1, c2, c3 = np.broadcast_arrays(*(np.asarray(c, dtype=np.uint64) & m32 for c in (c0, c1, c2, c3)))
    k0, k1 = np.uint64(k0 & 0xFFFFFFFF), np.uint64(k1 & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & m32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & m32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & m32, (k1 + np.uint64(0xBB67AE85)) & m32
    return c0, c1, c2, c3


def bf16_round(tensor: torch.Tensor) -> torch.Tensor:
    """float32 values rounded to bfloat16, round to nearest even, as float32 again: the rounding of a RANENV_NET_BF16 net's
    weights (once, at bind) and of its input and hidden activations (v_cvt_pk_bf16_f32 on the device).  On the bits, so it does
    not depend on the torch build: add 0x7FFF + (bit 16) and drop the low 16 bits."""
    x = torch.as_tensor(tensor).detach().to(torch.float32).contiguous()
    bits = x.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    out = ((bits + 0x7FFF + ((bits >> 16) & 1)) & 0xFFFF0000).to(torch.int64)
    out = torch.where(out >= 2 ** 31, out - 2 ** 32, out).to(torch.int32).view(torch.float32)
    return torch.where(torch.isnan(x), x, out)


def _mlp_forward(x: torch.Tensor, layers, activation: str, precision: str = "f32") -> torch.Tensor:
    """The float32 forward of a (W, b) stack.  ``precision`` "bf16" is the normative restatement of a RANENV_NET_BF16 net
    (include/ranenv.h): W and the input row rounded to bf16 (``bf16_round``), every hidden layer float32 accumulation + float32
    bias + float32 activation and then rounded to bf16, the output layer float32 and not rounded.  Products of bf16 numbers are
    exact in float32; the summation order is torch's here and the matrix core's on the device."""
    if precision not in ("f32", "bf16"):
        raise ValueError("precision must be 'f32' or 'bf16'")
    bf = precision == "bf16"
    act = torch.tanh if activation == "tanh" else torch.relu
    if bf:
        x = bf16_round(x)
    for i, (w, b) in enumerate(layers):
        x = x @ (bf16_round(w) if bf else w).t() + b
        if i < len(layers) - 1:
            x = act(x)
            if bf:
                x = bf16_round(x)
    return x


def ibsched_policy_actions(obs_inter, mask_inter, inter, obs_intra=None, mask_intra=None, intra=None, stochastic: bool = False,
                           seed: int = 0, intra_input: str = "obs", activation: Optional[str] = None, env_ids=None, episode=None,
                           step=None, precision: str = "f32"):
    """What the device computes under RANENV_POLICY_NETWORK, in plain torch / numpy (the normative statement the GPU tests
    compare against; include/ranenv.h spells out the same rules).

    ``obs_inter`` [B, 10*S], ``mask_inter`` [B, S]; ``obs_intra`` [B, S, 2*Us+9], ``mask_intra`` [B, S, Us] (intra net only);
    nets as for ``batched_env.policy_net_layers``.  Forward in float32, epilogue in float64:
      inter: (mean, log_std) = net(obs); with the sorted mask (``sorted_action_mask``) a masked position scores -1, the others
             clamp(mean, -1, 1), or when ``stochastic`` clamp(mean + exp(log_std) * z, -1, 1) with z = Box-Muller of Philox words
             0 and 1 at counter (env_ids + b, episode[b], step[b], POLICY_TAG + position), key = seed;
      intra: argmax of the 3 logits (lowest index on ties), or the categorical draw of Philox word 2 at (..., POLICY_TAG + slice).
    ``env_ids`` / ``episode`` / ``step``: [B] (the env's id base + index, views' episode_number and step_number before the TTI).
    ``intra`` may be a list of S nets (non-shared intra policies): slice index s's rows go through ``intra[s]``.
    ``precision`` "bf16": every net as bound with ``precision="bf16"`` (``_mlp_forward``).
    Returns (scores float64 [B, S], intra uint8 [B, S] or None) as CPU tensors."""
    from .batched_env import per_slice_nets, policy_net_layers
    obs_inter = torch.as_tensor(obs_inter).detach().cpu().to(torch.float32)
    B, S = obs_inter.shape[0], obs_inter.shape[1] // 10
    layers, act = policy_net_layers(inter, activation, 10 * S, 2 * S)
    out = _mlp_forward(obs_inter, [(w.cpu(), b.cpu()) for w, b in layers], act, precision).to(torch.float64)
    mean, log_std = out[:, :S], out[:, S:]
    masked = sorted_action_mask(torch.as_tensor(mask_inter).cpu()) == 0
    draws = None
    if stochastic:
        if env_ids is None or episode is None or step is None:
            raise ValueError("stochastic actions need env_ids, episode and step")
        col = lambda a: np.asarray(torch.as_tensor(a).cpu().numpy(), dtype=np.int64).reshape(B, 1)  # noqa: E731
        c3 = POLICY_TAG + np.arange(S, dtype=np.int64)[None, :]
        draws = philox4x32_10(col(env_ids), col(episode), col(step), c3, int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF)
        u1 = (draws[0].astype(np.float64) + 1.0) * 2.0 ** -32
        u2 = draws[1].astype(np.float64) * 2.0 ** -32
        z = torch.from_numpy(np.sqrt(-2.0 * np.log(u1)) * np.cos(6.283185307179586 * u2))
        mean = mean + torch.exp(log_std) * z
    scores = torch.where(masked, torch.full_like(mean, -1.0), mean.clamp(-1.0, 1.0))
    if intra is None:
        return scores, None
    obs_intra = torch.as_tensor(obs_intra).detach().cpu().to(torch.float32)
    Us = (obs_intra.shape[-1] - 9) // 2
    x = obs_intra.reshape(B * S, -1)
    if intra_input == "mask_obs":
        x = torch.cat([torch.as_tensor(mask_intra).cpu().reshape(B * S, Us).to(torch.float32), x], dim=1)
    elif intra_input != "obs":
        raise ValueError("intra_input must be 'obs' or 'mask_obs'")
    nets = per_slice_nets(intra)
    if nets is None:
        il, iact = policy_net_layers(intra, activation, x.shape[1], 3)
        lg = _mlp_forward(x, [(w.cpu(), b.cpu()) for w, b in il], iact, precision).reshape(B, S, 3)
    else:
        if len(nets) != S:
            raise ValueError(f"{len(nets)} intra nets given: one per slice is {S}")
        per = []
        for s, net in enumerate(nets):
            il, iact = policy_net_layers(net, activation, x.shape[1], 3)
            per.append(_mlp_forward(x.reshape(B, S, -1)[:, s], [(w.cpu(), b.cpu()) for w, b in il], iact, precision))
        lg = torch.stack(per, dim=1)
    if not stochastic:
        l0, l1, l2 = lg[..., 0], lg[..., 1], lg[..., 2]
        ch = (l1 > l0).to(torch.uint8)
        best = torch.where(l1 > l0, l1, l0)
        ch = torch.where(l2 > best, torch.full_like(ch, 2), ch)
        return scores, ch
    ld = lg.to(torch.float64)
    mx = ld.max(dim=-1, keepdim=True).values
    e = torch.exp(ld - mx)
    c0, c1 = e[..., 0], e[..., 0] + e[..., 1]
    t = torch.from_numpy(draws[2].astype(np.float64) * 2.0 ** -32) * (c1 + e[..., 2])
    ch = torch.where(t < c0, 0, torch.where(t < c1, 1, 2)).to(torch.uint8)
    return scores, ch


def ibsched_policy_noise(env_ids, episode, step, S: int, seed: int):
    """The policy's draws for [B] envs: (z float64 [B, S], the Box-Muller draw of position j; u float64 [B, S], the uniform of
    slice s's categorical draw), from Philox words 0 / 1 and 2 at counter (env id, episode, step, POLICY_TAG + j), key = seed."""
    col = lambda a: np.asarray(torch.as_tensor(a).cpu().numpy(), dtype=np.int64).reshape(-1, 1)  # noqa: E731
    c3 = POLICY_TAG + np.arange(S, dtype=np.int64)[None, :]
    d = philox4x32_10(col(env_ids), col(episode), col(step), c3, int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF)
    u1 = (d[0].astype(np.float64) + 1.0) * 2.0 ** -32
    u2 = d[1].astype(np.float64) * 2.0 ** -32
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(6.283185307179586 * u2), d[2].astype(np.float64) * 2.0 ** -32


HALF_LN_2PI = 0.9189385332046727      # 0.5 ln(2 pi)
LN_1E9 = 20.72326583694641            # ln(1e9)


def ibsched_policy_logp(inter_out, mask_inter, z=None, logits=None, choice=None):
    """The log-probabilities ``collect()`` records, restated in numpy float64 (include/ranenv.h has the same rules).

    ``inter_out`` float32 [B, 2S] = the inter net's (mean | log_std), ``mask_inter`` [B, S], ``z`` [B, S] the draws the actions
    used (None = the mode: z = 0):  sum over the active sorted positions j, ascending, of ((-0.5 z_j) z_j - log_std_j) - 0.5 ln 2 pi,
    then + n_masked (ln 1e9 - 0.5 ln 2 pi) -- TorchDiagGaussian.logp of agents/masked_action_distribution.py:30-36,53-54 at the
    action mean + exp(log_std) z (masked: Normal(-1, 1e-9) at exactly -1).
    ``logits`` float32 [B, S, 3] with ``choice`` [B, S]: (l_c - max l) - ln(sum_i exp(l_i - max l)).
    Returns (logp_inter float32 [B], logp_intra float32 [B, S] or None) as numpy arrays (float64 rounded once)."""
    as_np = lambda a, dt: np.asarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a, dtype=dt)  # noqa: E731
    out = as_np(inter_out, np.float64)
    S = out.shape[1] // 2
    ls = out[:, S:]
    active = sorted_action_mask(torch.as_tensor(as_np(mask_inter, np.int64))).numpy() != 0
    zz = np.zeros_like(ls) if z is None else as_np(z, np.float64)
    lp = np.zeros(out.shape[0], dtype=np.float64)
    for j in range(S):                                          # ascending positions, as the kernel sums them
        lp = lp + np.where(active[:, j], ((-0.5 * zz[:, j]) * zz[:, j] - ls[:, j]) - HALF_LN_2PI, 0.0)
    lp = lp + (S - active.sum(axis=1)).astype(np.float64) * (LN_1E9 - HALF_LN_2PI)
    lp_intra = None
    if logits is not None:
        lg = as_np(logits, np.float64)
        mx = lg.max(axis=-1)
        tot = (np.exp(lg[..., 0] - mx) + np.exp(lg[..., 1] - mx)) + np.exp(lg[..., 2] - mx)
        lc = np.take_along_axis(lg, as_np(choice, np.int64)[..., None], -1)[..., 0]
        lp_intra = ((lc - mx) - np.log(tot)).astype(np.float32)
    return lp.astype(np.float32), lp_intra


def gae(reward, vf, done, gamma: float = 0.99, lam: float = 0.95):
    """Generalised advantage estimation as the device computes it (ranenv_collect / ranenv_gae), in numpy float64 with the same
    operations in the same order: ``reward`` [T, B, C], ``vf`` [T + 1, B, C] (slot T = bootstrap), ``done`` [T, B] ->
    (adv, vtarg) float32 [T, B, C].  ``done`` is terminal as in the reference (simu.py:559-564): nothing is carried across it."""
    as_np = lambda a, dt: np.asarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a, dtype=dt)  # noqa: E731
    r, v, d = as_np(reward, np.float64), as_np(vf, np.float64), as_np(done, np.uint8)
    T = r.shape[0]
    adv, vtarg = np.empty(r.shape, dtype=np.float32), np.empty(r.shape, dtype=np.float32)
    a_next = np.zeros(r.shape[1:], dtype=np.float64)
    gamma, gl = float(gamma), float(gamma) * float(lam)
    for t in range(T - 1, -1, -1):
        nd = np.where(d[t] != 0, 0.0, 1.0)[:, None]
        delta = (r[t] + (gamma * v[t + 1]) * nd) - v[t]
        a = delta + (gl * nd) * a_next
        adv[t] = a.astype(np.float32)
        vtarg[t] = (a + v[t]).astype(np.float32)
        a_next = a
    return adv, vtarg


# --------------------------------------------------------------------------------------------
# the PPO update (ranenv_ppo_update, include/ranenv.h "PPO update"): the shuffles it takes and its float64 restatement
# --------------------------------------------------------------------------------------------
HALF_LN_2PI = 0.9189385332046727
LN_1E9 = 20.72326583694641


def ppo_row_order(rec, first_env, epochs: int, seed: int = 0, intra: bool = True, per_slice: bool = False) -> Dict[str, object]:
    """The row lists of ``ppo_update`` for a ``collect()`` record: per epoch and member an independent shuffle of the member's rows,
    built where the record lives in one batched ``argsort`` per kind.  ``first_env`` [G + 1]: the population's grouping (``[0, B]``: one
    member).  Inter rows are ``t * B + b`` for every TTI t and env b of the member; intra rows ``(t * B + b) * S + s`` for the slices
    that were live at that TTI (``mask_inter != 0``) only.  Returns ``order_inter`` int32 [epochs, N_inter] and ``first_inter`` int32
    [G + 1] (member m's rows of an epoch: entries ``first[m] .. first[m + 1] - 1``), and the same for "intra" (None with ``intra=False``).
    ``per_slice=True`` (``ppo_update_per_slice``, non-shared intra policies; one member only): the live intra rows are grouped by
    slice and shuffled within it, and ``first_intra`` is [S + 1] -- slice s's share of an epoch is entries ``first_intra[s] ..
    first_intra[s + 1] - 1``, every one a row of slice s.  ``order_inter`` is the same tensor either way for one seed."""
    mask = rec["mask_inter"]
    T, B, S = mask.shape
    dev = mask.device
    first = np.asarray(first_env, dtype=np.int64)
    G = len(first) - 1
    if first[0] != 0 or first[-1] != B or np.any(np.diff(first) <= 0):
        raise ValueError(f"first_env runs from 0 to {B} strictly increasing")
    member_of_env = torch.repeat_interleave(torch.arange(G, device=dev), torch.as_tensor(np.diff(first), device=dev))
    gen = torch.Generator(device=dev)
    gen.manual_seed(int(seed))

    if per_slice and G != 1:
        raise ValueError("per_slice=True takes one member: there is no population of non-shared agents")

    def shuffled(rows, member, G=G):          # rows ascending; member [n] of each
        counts = torch.bincount(member, minlength=G).cpu().numpy()
        by_member = torch.argsort(member, stable=True)
        rows, member = rows[by_member], member[by_member]
        keys = (member.to(torch.int64) << 32)[None, :] + torch.randint(0, 2 ** 31, (int(epochs), rows.numel()), generator=gen, device=dev)
        # (31 random bits per row tie now and then; a stable sort makes "same seed, same order" independent of the sort's tie handling)
        order = rows[torch.argsort(keys, dim=1, stable=True)].to(torch.int32).contiguous()
        return order, np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)

    rows = torch.arange(T * B, device=dev)
    out = {"order_intra": None, "first_intra": None}
    out["order_inter"], out["first_inter"] = shuffled(rows, member_of_env[rows % B])
    if intra:
        rows = (mask != 0).reshape(-1).nonzero().squeeze(1)
        out["order_intra"], out["first_intra"] = shuffled(rows, rows % S, S) if per_slice else shuffled(rows, member_of_env[(rows // S) % B])
    return out


ROWS_TAG = 0x53485546            # "SHUF": counter word c3 of the row lists' Philox keys, + block (include/ranenv.h "Row lists on the device")
PPO_ROWS_MEMBERS, PPO_ROWS_SLICES = 0, 1


PPO_ROW_SLIPS = ("no_cycle_walk", "no_unit", "no_epoch", "member_shift", "slice_div", "keep_masked")


def ppo_row_permutation(n: int, seed: int, epoch: int, unit: int, kind: int, slip: Optional[str] = None) -> np.ndarray:
    """THE NORMATIVE STATEMENT of the device row lists' shuffle (ranenv_ppo_row_order, include/ranenv.h "Row lists on the device"):
    the keyed bijection P of ``[0, n)`` for (``seed``, ``epoch``, ``unit``, ``kind`` 0 inter / 1 intra) as int64 [n], numpy,
    vectorised over the positions.  An eight-round Feistel network on the 2h-bit domain that covers n (h = max(1,
    ceil(bit_length(n - 1) / 2))), round function murmur3's finaliser of (R + key[r]), keys the eight words of two Philox-4x32-10
    blocks at counter (epoch, unit, kind, "SHUF" + block) under the seed's two words; a position that leaves ``[0, n)`` takes the
    pass again (cycle walking).  Nothing is sorted, and entry i needs nothing but i.  ``slip``: a planted mistake for the tests
    ("no_cycle_walk": one pass, values clamped into the range; "no_unit" / "no_epoch": that word left out of the counter)."""
    n = int(n)
    if slip == "no_unit":
        unit = 0
    if slip == "no_epoch":
        epoch = 0
    if n < 1:
        return np.zeros(0, dtype=np.int64)
    if n == 1:
        return np.zeros(1, dtype=np.int64)
    h = max(1, -(-int(n - 1).bit_length() // 2))
    m32, mask, hh = np.uint64(0xFFFFFFFF), np.uint64((1 << h) - 1), np.uint64(h)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    keys = []
    for j in range(2):
        keys += [np.uint64(int(w)) for w in philox4x32_10(int(epoch), int(unit), int(kind), ROWS_TAG + j, seed & 0xFFFFFFFF, seed >> 32)]

    def one_pass(x):
        left, right = x >> hh, x & mask
        for r in range(8):
            f = (right + keys[r]) & m32
            f ^= f >> np.uint64(16)
            f = (f * np.uint64(0x85EBCA6B)) & m32
            f ^= f >> np.uint64(13)
            f = (f * np.uint64(0xC2B2AE35)) & m32
            f ^= f >> np.uint64(16)
            left, right = right, left ^ (f & mask)
        return (left << hh) | right

    x = one_pass(np.arange(n, dtype=np.uint64))
    if slip == "no_cycle_walk":
        return np.minimum(x, np.uint64(n - 1)).astype(np.int64)
    while True:
        out = np.nonzero(x >= np.uint64(n))[0]
        if out.size == 0:
            return x.astype(np.int64)
        x[out] = one_pass(x[out])


def ppo_row_order_reference(mask_inter, first_env, epochs: int, seed: int, intra: bool = True, per_slice: bool = False,
                            slip: Optional[str] = None) -> Dict[str, object]:
    """The numpy twin of ``BatchedRanEnv.ppo_row_order`` (ranenv_ppo_row_count + ranenv_ppo_row_order): ``adapters.ppo_row_order``'s
    dict as numpy arrays -- ``order_<kind>`` int32 [epochs, N_kind], ``first_<kind>`` int32 [units + 1] -- for the record's
    ``mask_inter`` [T, B, S] (with ``intra=False`` a ``(T, B, S)`` shape will do: no mask is read).  Unit u's base list is its inter
    rows ``t * B + b`` or its live intra cells ``(t * B + b) * S + s`` in ascending order -- the units are the members of
    ``first_env``, or with ``per_slice=True`` (one member only) the one inter agent and the S slices -- and epoch k's entries
    ``first[u] + i`` are ``base_u[ppo_row_permutation(n_u, seed, k, u, kind)[i]]``.  ``slip``: one of ``PPO_ROW_SLIPS``, a planted
    mistake for the tests (the permutation's three; "member_shift": the members' inner boundaries one env late; "slice_div": the
    slices' grouping by ``cell // S % S``; "keep_masked": a compaction that keeps every cell)."""
    if isinstance(mask_inter, tuple):
        if intra:
            raise ValueError("the intra lists read mask_inter: a shape alone gives the inter lists")
        (T, B, S), mask = (int(x) for x in mask_inter), None
    else:
        mask = mask_inter.detach().cpu().numpy() if isinstance(mask_inter, torch.Tensor) else np.asarray(mask_inter)
        T, B, S = mask.shape
    if T * B * S > 2 ** 31 - 1:
        raise ValueError("the record is limited to T * B * S <= 2^31 - 1 cells")
    first = np.asarray(first_env, dtype=np.int64)
    G = len(first) - 1
    if first[0] != 0 or first[-1] != B or np.any(np.diff(first) <= 0):
        raise ValueError(f"first_env runs from 0 to {B} strictly increasing")
    if per_slice and G != 1:
        raise ValueError("per_slice=True takes one member: there is no population of non-shared agents")
    epochs = int(epochs)
    if slip is not None and slip not in PPO_ROW_SLIPS:
        raise ValueError(f"slip: one of {PPO_ROW_SLIPS}")
    if slip == "member_shift":
        first = np.concatenate([first[:1], np.minimum(first[1:-1] + 1, B), first[-1:]])

    def lists(bases, kind):
        counts = [len(b) for b in bases]
        firsts = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
        order = np.zeros((epochs, int(firsts[-1])), dtype=np.int32)
        for u, base in enumerate(bases):
            for k in range(epochs):
                if len(base):
                    order[k, firsts[u]:firsts[u + 1]] = base[ppo_row_permutation(len(base), seed, k, u, kind, slip)]
        return order, firsts

    t_rows = np.arange(T, dtype=np.int64)[:, None] * B
    out = {"order_intra": None, "first_intra": None}
    out["order_inter"], out["first_inter"] = lists([(t_rows + np.arange(first[m], first[m + 1])[None, :]).reshape(-1) for m in range(G)], 0)
    if intra:
        cells = np.arange(T * B * S, dtype=np.int64) if slip == "keep_masked" else np.nonzero(mask.reshape(-1) != 0)[0].astype(np.int64)
        unit = ((cells // S) % S if slip == "slice_div" else cells % S) if per_slice else np.searchsorted(first, (cells // S) % B, side="right") - 1
        out["order_intra"], out["first_intra"] = lists([cells[unit == u] for u in range(S if per_slice else G)], 1)
    return out


def ppo_rows(rec, kind: str, rows, layout: str = "obs", dtype=torch.float64) -> Dict[str, torch.Tensor]:
    """The record rows ``rows`` (``ppo_row_order``'s numbering) of ``kind`` "inter" / "intra" as the update reads them: the net input
    "x", the recorded action ("action" [n, S] with the sorted mask "active", or "choice" [n]) and "logp", "adv", "vtarg" of the row's column."""
    rows = torch.as_tensor(rows, dtype=torch.int64, device=rec["logp"].device)
    S = rec["mask_inter"].shape[-1]
    cols = lambda name, r, c: rec[name][:rec["logp"].shape[0]].reshape(-1, S + 1)[r, c].to(dtype)  # noqa: E731
    if kind == "inter":
        out = {"x": rec["obs_inter"].reshape(-1, 10 * S)[rows].to(dtype), "action": rec["action_inter"].reshape(-1, S)[rows].to(dtype),
               "active": sorted_action_mask(rec["mask_inter"].reshape(-1, S)[rows]) != 0}
        r, c = rows, torch.zeros_like(rows)
    else:
        W = rec["obs_intra"].shape[-1]
        x = rec["obs_intra"].reshape(-1, W)[rows].to(dtype)
        if layout == "mask_obs":
            x = torch.cat([rec["mask_intra"].reshape(-1, rec["mask_intra"].shape[-1])[rows].to(dtype), x], dim=1)
        out = {"x": x, "choice": rec["action_intra"].reshape(-1)[rows].to(torch.int64)}
        r, c = rows // S, 1 + rows % S
    out.update(logp=cols("logp", r, c), adv=cols("adv", r, c), vtarg=cols("vtarg", r, c))
    return out


PPO_BF16_SLIPS = ("bf16_trunc_d", "bf16_unrounded_d", "bf16_unrounded_dl", "bf16_act_unrounded", "bf16_master_backward", "bf16_stale_acting",
                  "bf16_wt_swapped")


def _bf16_of(x: torch.Tensor, mode: str = "rne") -> torch.Tensor:
    """``x`` rounded to bf16 in its own dtype: "rne" (``bf16_round``), "trunc" (the low 16 bits dropped: a planted slip) or "none"."""
    if mode == "none":
        return x
    if mode == "rne":
        return bf16_round(x).to(x.dtype)
    bits = x.detach().to(torch.float32).contiguous().view(torch.int32) & -65536
    return bits.view(torch.float32).to(x.dtype)


class _Bf16Linear(torch.autograd.Function):
    """Contract steps 1 and 3 of one layer of a bf16-trained net: forward ``a @ bf16(W).T + b`` on the acting copy (``wq`` given: that
    copy, else the master ``w`` rounded); backward with the incoming D_l: dW = D_l^T a to the MASTER (the rounding has derivative 1),
    db the column sums, and D_l Wq to the input.  ``slip``: the product on the master, or on a copy whose k columns are swapped in pairs."""
    @staticmethod
    def forward(ctx, a, w, b, wq, slip):
        wq = bf16_round(w).to(w.dtype) if wq is None else wq
        ctx.save_for_backward(a, w, wq)
        ctx.slip = slip
        return a @ wq.t() + b

    @staticmethod
    def backward(ctx, g):
        a, w, wq = ctx.saved_tensors
        wb = w if ctx.slip == "bf16_master_backward" else wq
        if ctx.slip == "bf16_wt_swapped":
            k = torch.arange(wb.shape[1])
            wb = wb[:, torch.where((k ^ 1) < wb.shape[1], k ^ 1, k)]
        return g @ wb, g.t() @ a, g.sum(dim=0), None, None


class _Bf16Act(torch.autograd.Function):
    """A hidden layer's activation under the contract: a = bf16(act(z)); backward D = bf16(g * act'(a)), act' from the ROUNDED value,
    one rounding behind the product.  ``slip``: D truncated or unrounded, act' from the unrounded value."""
    @staticmethod
    def forward(ctx, z, act, slip):
        y = torch.tanh(z) if act == "tanh" else torch.relu(z)
        a = _bf16_of(y)
        ctx.save_for_backward(y if slip == "bf16_act_unrounded" else a)
        ctx.act, ctx.slip = act, slip
        return a

    @staticmethod
    def backward(ctx, g):
        s, = ctx.saved_tensors
        d = 1.0 - s * s if ctx.act == "tanh" else (s > 0).to(s.dtype)
        return _bf16_of(g * d, {"bf16_trunc_d": "trunc", "bf16_unrounded_d": "none"}.get(ctx.slip, "rne")), None, None


class _Bf16Grad(torch.autograd.Function):
    """Identity whose gradient is rounded to bf16 on the way back: D_L = bf16(G) at the output layer (``mode`` "none": a slip)."""
    @staticmethod
    def forward(ctx, x, mode):
        ctx.mode = mode
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return _bf16_of(g, ctx.mode), None


def _mlp_forward_bf16_trained(x: torch.Tensor, layers, activation: str, acting=None, slip: Optional[str] = None) -> torch.Tensor:
    """The forward of a bf16-trained net on its MASTER ``layers`` whose autograd backward is contract step 3 (include/ranenv.h "bf16 nets
    over the chip"); in float32 its value is ``_mlp_forward(..., precision="bf16")``'s bit for bit.  ``acting``: the acting copy's
    ``(Wq, b)`` where it is not bf16 of the masters (the stale-copy slip)."""
    a = _bf16_of(x)
    for i, (w, b) in enumerate(layers):
        z = _Bf16Linear.apply(a, w, b, None if acting is None else acting[i][0], slip)
        if i < len(layers) - 1:
            a = _Bf16Act.apply(z, activation, slip)
    return _Bf16Grad.apply(z, "none" if slip == "bf16_unrounded_dl" else "rne")


def ppo_loss_reference(actor, critic, batch, kind: str, clip: float, vf_coeff: float, ent_coeff: float, adv_norm: bool, act_actor: str = "tanh",
                       act_critic: str = "tanh", slip: Optional[str] = None, precision: str = "f32", acting=None):
    """The minibatch loss of ``ppo_update`` in torch (autograd differentiates it): ``actor`` / ``critic`` (None: no value term) lists of
    ``(W, b)`` in the dtype to compute in, ``batch`` from ``ppo_rows``.  Returns (loss, {policy_loss, value_loss, entropy, kl,
    clip_frac, logp}).  ``slip``: a deliberately wrong variant, for the tests that show the tolerances bite.  ``precision`` "bf16":
    the nets are the MASTERS of a bf16-trained pair (``ppo_bind(spread=True, bf16=True)``): forward and backward are the numeric
    contract's (``_mlp_forward_bf16_trained``; ``slip`` one of ``PPO_BF16_SLIPS``, ``acting`` = (actor, critic) acting copies for the
    stale-copy slip); the loss on the outputs is the same."""
    if precision not in ("f32", "bf16"):
        raise ValueError("precision must be 'f32' or 'bf16'")

    def forward(x, layers, act, deriv=None):
        if precision == "bf16":
            return _mlp_forward_bf16_trained(x, layers, act, None if acting is None else acting[0 if layers is actor else 1], slip)
        for i, (w, b) in enumerate(layers):
            if slip == "db_drops_row_32" and i == 0 and x.shape[0] > 32:      # (row 32 misses layer 0's bias reduction)
                rows = b.expand(x.shape[0], -1)
                x = x @ w.T + torch.cat([rows[:32], rows[32:33].detach(), rows[33:]])
            else:
                x = x @ w.T + b
            if i < len(layers) - 1:
                y = torch.tanh(x) if act == "tanh" else torch.relu(x)
                if slip == "no_activation_derivative":
                    x = y.detach() + (x - x.detach())
                elif deriv is not None and deriv != act:      # (the other activation's derivative, from the output as the kernel takes it)
                    d = 1.0 - y * y if deriv == "tanh" else (y > 0).to(y.dtype)
                    x = y.detach() + (x - x.detach()) * d.detach()
                else:
                    x = y
        return x
    out = forward(batch["x"], actor, act_actor)
    if kind == "inter":
        S = batch["action"].shape[1]
        mean, ls = out[:, :S], out[:, S:]
        active = torch.ones_like(batch["active"]) if slip == "masked_gradient" else batch["active"]
        z = (batch["action"] - mean) / torch.exp(ls)
        zero = torch.zeros_like(z)
        logp = torch.where(active, (-0.5 * z) * z - ls - HALF_LN_2PI, zero).sum(dim=1) + (~batch["active"]).sum(dim=1).to(z.dtype) * (LN_1E9 - HALF_LN_2PI)
        entropy = torch.where(active, ls + 0.5 + HALF_LN_2PI, zero).sum(dim=1)
    else:
        lsm = torch.log_softmax(out, dim=1)
        logp = lsm.gather(1, batch["choice"][:, None])[:, 0]
        entropy = -(torch.exp(lsm) * lsm).sum(dim=1)
    adv, n = batch["adv"], batch["adv"].numel()
    if adv_norm:
        adv = (adv - adv.mean()) / ((adv.std() if n > 1 else torch.zeros((), dtype=adv.dtype)) + 1e-8)
    mean_of = (lambda v: v.sum() / 32.0) if slip == "mean_over_32" else (lambda v: v.mean())
    ratio = torch.exp(logp - batch["logp"])
    surrogate = ratio * adv if slip == "unclipped" else torch.minimum(ratio * adv, ratio.clamp(1.0 - clip, 1.0 + clip) * adv)
    stats = {"policy_loss": -mean_of(surrogate), "entropy": mean_of(entropy), "kl": mean_of(batch["logp"] - logp),
             "clip_frac": mean_of(((ratio < 1.0 - clip) | (ratio > 1.0 + clip)).to(ratio.dtype)), "logp": logp, "value_loss": torch.zeros((), dtype=ratio.dtype)}
    loss = stats["policy_loss"] - (-ent_coeff if slip == "entropy_sign" else ent_coeff) * stats["entropy"]
    if critic is not None:
        stats["value_loss"] = mean_of((forward(batch["x"], critic, act_critic, act_actor if slip == "critic_takes_actor_derivative" else None)[:, 0] - batch["vtarg"]) ** 2)
        loss = loss + vf_coeff * stats["value_loss"]
    return loss, stats


def ppo_adam_reference(params, grads, state, lr: float, grad_clip: float, betas=(0.9, 0.999), eps: float = 1e-8, slip: Optional[str] = None):
    """Joint gradient clip (``clip_grad_norm_``: scale = min(1, grad_clip / (norm + 1e-6)); ``grad_clip`` <= 0: none) and one Adam step
    in torch.optim.Adam's operation order, in the tensors' dtype and in place: ``params`` / ``grads`` lists of tensors, ``state``
    {"m": [...], "v": [...], "t": int} (empty dict: a new optimiser).  Returns the pre-clip norm."""
    if not state:
        state.update(m=[torch.zeros_like(p) for p in params], v=[torch.zeros_like(p) for p in params], t=0)
    norm = torch.sqrt(sum((g.to(torch.float64) ** 2).sum() for g in grads))
    scale = min(1.0, grad_clip / (float(norm) + 1e-6)) if grad_clip > 0 else 1.0
    state["t"] += 1
    b1, b2, t = betas[0], betas[1], state["t"]
    bc1, bc2 = (1.0, 1.0) if slip == "no_bias_correction" else (1.0 - b1 ** t, 1.0 - b2 ** t)
    for p, g, m, v in zip(params, grads, state["m"], state["v"]):
        g = g * scale
        m.mul_(b1).add_((1.0 - b1) * g)
        v.mul_(b2).add_(((1.0 - b2) * g) * g)
        p.sub_((lr / bc1) * (m / (torch.sqrt(v) / np.sqrt(bc2) + eps)))
    return float(norm)


def ppo_update_reference(rec, kind: str, actor, critic, order, lo: int, hi: int, epochs: int = 10, minibatch: int = 64, lr: float = 3e-4,
                         clip: float = 0.2, vf_coeff: float = 0.5, ent_coeff: float = 0.01, grad_clip: float = 0.5, adv_norm: bool = True,
                         betas=(0.9, 0.999), eps: float = 1e-8, act_actor: str = "tanh", act_critic: str = "tanh", layout: str = "obs",
                         state: Optional[dict] = None, dtype=torch.float64, slip: Optional[str] = None, precision: str = "f32"):
    """THE NORMATIVE STATEMENT of ``ppo_update`` for one member and kind, float64 torch autograd on the CPU: ``actor`` / ``critic`` lists
    of ``(W, b)`` (copied), the member's rows of epoch k are ``order[k, lo:hi]``, minibatches consecutive chunks of ``minibatch`` with a
    short last one.  Returns {"actor", "critic": the trained layers, "state": Adam's, "stats": float64 [epochs, 8] as ``_lib.PPO_STATS``,
    "grad": the last minibatch's unclipped gradients as lists of (dW, db) for actor and critic}.
    ``precision`` "bf16": the twin of ``ppo_bind(spread=True, bf16=True)`` -- ``actor`` / ``critic`` are the MASTER weights, kept in
    ``dtype``; every pass runs the header's numeric contract on the acting copy bf16(master) (``ppo_loss_reference``), Adam steps the
    masters, and the acting copy is re-rounded from them behind every optimiser step, so it is the multi-step twin too; the result
    has "acting": {"actor", "critic"}, the acting copies behind the last step.  The default "f32" is the path above, untouched."""
    if precision not in ("f32", "bf16"):
        raise ValueError("precision must be 'f32' or 'bf16'")
    rounded = lambda net: None if net is None else [(_bf16_of(w.detach()), b.detach().clone()) for w, b in net]  # noqa: E731
    cpu = {k: v.detach().cpu() for k, v in rec.items() if isinstance(v, torch.Tensor)}
    order = torch.as_tensor(order).cpu().to(torch.int64)
    copy = lambda net: None if net is None else [(w.detach().cpu().to(dtype).clone().requires_grad_(True), b.detach().cpu().to(dtype).clone().requires_grad_(True))  # noqa: E731
                                                  for w, b in net]
    actor, critic = copy(actor), copy(critic)
    params = [p for net in (actor, critic) if net is not None for wb in net for p in wb]
    stale = (rounded(actor), rounded(critic)) if slip == "bf16_stale_acting" else None      # (the acting copy never re-rounded: a slip)
    state = {} if state is None else state
    stats, grads = np.zeros((epochs, 8)), None
    n = hi - lo
    for ep in range(epochs):
        acc = np.zeros(6)
        n_mb = 0
        for c0 in range(0, n, minibatch):
            rows = order[ep, lo + c0:lo + min(c0 + minibatch, n)]
            batch = ppo_rows(cpu, kind, rows, layout, dtype)
            loss, st = ppo_loss_reference(actor, critic, batch, kind, clip, vf_coeff, ent_coeff, adv_norm, act_actor, act_critic, slip, precision, stale)
            grads = torch.autograd.grad(loss, params)
            with torch.no_grad():
                norm = ppo_adam_reference(params, list(grads), state, lr, grad_clip, betas, eps, slip)
            nb = rows.numel()
            acc += nb * np.array([float(st[k].detach()) for k in ("policy_loss", "value_loss", "entropy", "kl", "clip_frac")] + [norm])
            n_mb += 1
        stats[ep, :6], stats[ep, 6], stats[ep, 7] = acc / n, n, n_mb
    pairs = lambda flat: [(flat[2 * i], flat[2 * i + 1]) for i in range(len(flat) // 2)]  # noqa: E731
    na = 2 * len(actor)
    out = {"actor": [(w.detach(), b.detach()) for w, b in actor], "critic": None if critic is None else [(w.detach(), b.detach()) for w, b in critic],
           "state": state, "stats": stats, "grad": {"actor": pairs(list(grads[:na])), "critic": pairs(list(grads[na:]))}}
    if precision == "bf16":
        out["acting"] = {"actor": stale[0] if stale else rounded(actor), "critic": stale[1] if stale else rounded(critic)}
    return out


# --------------------------------------------------------------------------------------------
# the PPO update of the head policies (ranenv_ppo_update_head, include/ranenv.h): its shuffles and its float64 restatement
# --------------------------------------------------------------------------------------------
def ppo_head_row_order(rec, epochs: int, seed: int = 0) -> torch.Tensor:
    """The row lists of ``ppo_update_head`` for a ``collect_head()`` record: int32 [epochs, T * B], per epoch an independent
    permutation of the record rows ``t * B + b``, drawn where the record lives from ``seed``."""
    T, B = rec["logp"].shape[:2]
    dev = rec["logp"].device
    gen = torch.Generator(device=dev)
    gen.manual_seed(int(seed))
    # (31 random bits per row tie now and then; a stable sort makes "same seed, same order" independent of the sort's tie handling)
    keys = torch.randint(0, 2 ** 31, (int(epochs), int(T) * int(B)), generator=gen, device=dev)
    return torch.argsort(keys, dim=1, stable=True).to(torch.int32).contiguous()


def ppo_head_update_reference(rec, actor, log_std, critic, order, epochs: int = 10, minibatch: int = 64, lr: float = 3e-4, clip: float = 0.2,
                              vf_coeff: float = 0.5, ent_coeff: float = 0.0, grad_clip: float = 0.5, adv_norm: bool = True, betas=(0.9, 0.999),
                              eps: float = 1e-5, act_actor: str = "tanh", act_critic: str = "tanh", state: Optional[dict] = None,
                              dtype=torch.float64, slip: Optional[str] = None):
    """THE NORMATIVE STATEMENT of ``ppo_update_head``, torch autograd on the CPU (float64 unless ``dtype``): SB3's ``PPO.train`` with
    ``clip_range_vf=None`` on a ``collect_head()`` record -- ``actor`` / ``critic`` lists of ``(W, b)`` (copied), ``log_std`` [S] an
    ``nn.Parameter`` of a diagonal Gaussian over ALL S positions, the joint clip ``clip_grad_norm_`` over actor, critic and ``log_std``,
    Adam over the three with one counter (``ppo_adam_reference``: torch.optim.Adam's order).  Epoch k's rows are ``order[k]``,
    minibatches consecutive chunks of ``minibatch`` with a short last one; every entry must lie inside the record.  "kl" is this
    project's mean(logp_old - logp), not SB3's logged estimator; a one-row minibatch under ``adv_norm`` gets advantage 0 (SB3 skips the
    normalisation there).  Returns {"actor", "critic": the trained layers, "log_std", "state": Adam's (params in the order actor,
    critic, log_std), "stats": float64 [epochs, 8] as ``_lib.PPO_STATS``, "grad": {"actor": [(dW, db)], "critic": [...], "log_std"} of the
    last minibatch, unclipped, "logp": the last minibatch's re-evaluated log-probabilities, "clip_fracs": every minibatch's}.
    ``slip``: a deliberately wrong variant, for the tests that show the tolerances bite."""
    cpu = {k: v.detach().cpu() for k, v in rec.items() if isinstance(v, torch.Tensor)}
    order = torch.as_tensor(order).cpu().to(torch.int64)
    leaf = lambda x: torch.as_tensor(x).detach().cpu().to(dtype).clone().requires_grad_(True)  # noqa: E731
    actor, critic = [(leaf(w), leaf(b)) for w, b in actor], [(leaf(w), leaf(b)) for w, b in critic]
    log_std = torch.nn.Parameter(torch.as_tensor(log_std).detach().cpu().to(dtype).clone())
    log_std0 = log_std.detach().clone()
    S = log_std.numel()
    T = cpu["logp"].shape[0]
    n_record = T * cpu["logp"].shape[1]
    obs, action = cpu["obs_head"].reshape(n_record, 10 * S).to(dtype), cpu["action"].reshape(n_record, S).to(dtype)
    cell = lambda name: cpu[name][:T].reshape(-1).to(dtype)  # noqa: E731
    logp_old, adv_all, vtarg = cell("logp"), cell("adv"), cell("vtarg")
    params = [p for net in (actor, critic) for wb in net for p in wb] + [log_std]
    state = {} if state is None else state

    def forward(x, layers, act):
        for i, (w, b) in enumerate(layers):
            x = x @ w.T + b
            if i < len(layers) - 1:
                x = torch.tanh(x) if act == "tanh" else torch.relu(x)
        return x

    stats, grads, logp, clip_fracs = np.zeros((epochs, 8)), None, None, []
    n, step = order.shape[1], 0
    for ep in range(epochs):
        acc, n_mb = np.zeros(6), 0
        for c0 in range(0, n, minibatch):
            rows = order[ep, c0:min(c0 + minibatch, n)]
            nb = rows.numel()
            cells = (rows * (S + 1)) % n_record if slip == "cell_stride" else rows      # (the IBSched record's column 0)
            ls = log_std0 + (log_std - log_std.detach()) if slip == "stale_log_std" and step >= 1 else log_std
            mean = forward(obs[rows], actor, act_actor)
            dist = torch.distributions.Normal(mean, torch.exp(ls).expand_as(mean))
            terms = dist.log_prob(action[rows])
            if slip == "short_logp":
                terms = terms[:, :S - 1]
            elif slip == "masked_term":                      # (the inter kind with position 0 masked)
                terms = torch.cat([torch.full_like(terms[:, :1], LN_1E9 - HALF_LN_2PI), terms[:, 1:]], dim=1)
            logp = terms.sum(dim=1)
            ent_ls = ls.detach() if slip == "no_entropy_gradient" else ls
            entropy = torch.distributions.Normal(mean, torch.exp(ent_ls).expand_as(mean)).entropy().sum(dim=1)
            adv = adv_all[cells]
            if adv_norm:
                adv = (adv - adv.mean()) / ((adv.std() if nb > 1 else torch.zeros((), dtype=dtype)) + 1e-8)
            ratio = torch.exp(logp - logp_old[cells])
            surrogate = torch.minimum(ratio * adv, ratio.clamp(1.0 - clip, 1.0 + clip) * adv)
            value_loss = ((forward(obs[rows], critic, act_critic)[:, 0] - vtarg[cells]) ** 2).mean()
            policy_loss, ent = -surrogate.mean(), entropy.mean()
            loss = policy_loss + vf_coeff * value_loss - ent_coeff * ent
            for p in params:
                p.grad = None
            loss.backward()
            grads = [p.grad.detach().clone() for p in params]
            clipped = params[:-1] if slip == "log_std_outside_norm" else params
            norm = float(torch.nn.utils.clip_grad_norm_(clipped, grad_clip if grad_clip > 0 else float("inf")))
            with torch.no_grad():
                ppo_adam_reference(params, [p.grad for p in params], state, lr, 0.0, betas, eps)
            cf = float(((ratio < 1.0 - clip) | (ratio > 1.0 + clip)).to(dtype).mean())
            clip_fracs.append(cf)
            acc += nb * np.array([float(x.detach()) for x in (policy_loss, value_loss, ent, (logp_old[cells] - logp).mean())] + [cf, norm])
            n_mb += 1
            step += 1
        stats[ep, :6], stats[ep, 6], stats[ep, 7] = acc / n, n, n_mb
    pairs = lambda flat: [(flat[2 * i], flat[2 * i + 1]) for i in range(len(flat) // 2)]  # noqa: E731
    na, nc = 2 * len(actor), 2 * len(critic)
    return {"actor": [(w.detach(), b.detach()) for w, b in actor], "critic": [(w.detach(), b.detach()) for w, b in critic],
            "log_std": log_std.detach(), "state": state, "stats": stats,
            "grad": {"actor": pairs(grads[:na]), "critic": pairs(grads[na:na + nc]), "log_std": grads[-1]},
            "logp": None if logp is None else logp.detach(), "clip_fracs": clip_fracs}


def sb3_ppo_state_dict(actor_layers, log_std, critic_layers):
    """The inverse of ``sb3_ppo_layers``: an SB3 ``PPO`` ``MlpPolicy`` state dict (separate pi / vf ``net_arch``) from the actor layers,
    ``log_std`` [S] and the critic layers, e.g. ``head_net_weights("actor")``, ``head_log_std()``, ``head_net_weights("critic")`` after
    ``ppo_update_head``: ``sb3_ppo_layers(sb3_ppo_state_dict(a, ls, c))`` returns the same tensors.  Key names restated from SB3's
    documented module layout: parity with SB3 itself is unpinned, no real checkpoint has been written or read."""
    if len(actor_layers) < 2 or len(critic_layers) < 2:
        raise ValueError("an MlpPolicy has at least one hidden layer in front of action_net / value_net")
    out = {"log_std": torch.as_tensor(log_std).detach().clone()}
    for prefix, last, layers in (("mlp_extractor.policy_net.", "action_net", actor_layers), ("mlp_extractor.value_net.", "value_net", critic_layers)):
        for i, (w, b) in enumerate(layers[:-1]):
            out[f"{prefix}{2 * i}.weight"], out[f"{prefix}{2 * i}.bias"] = torch.as_tensor(w).detach().clone(), torch.as_tensor(b).detach().clone()
        out[f"{last}.weight"], out[f"{last}.bias"] = torch.as_tensor(layers[-1][0]).detach().clone(), torch.as_tensor(layers[-1][1]).detach().clone()
    return out


def rllib_per_slice_layers(weights_by_policy, S: int, policy_prefix: str = "intra_slice_sched_"):
    """The S intra policies of a non-shared IBSched checkpoint (agents/ray_agent.py:432-460) from ``{policy_id: state_dict}`` as
    ``Algorithm.get_weights()`` returns it: ``(actors, critics)``, two lists of S layer stacks in slice order -- entry s from
    policy ``{policy_prefix}{s}``, which acts for ``player_{s+1}`` -- read with ``rllib_fcnet_layers`` /
    ``rllib_fcnet_value_layers``.  A missing policy raises KeyError naming it."""
    actors, critics = [], []
    for s in range(int(S)):
        name = f"{policy_prefix}{s}"
        if name not in weights_by_policy:
            raise KeyError(name)
        actors.append(rllib_fcnet_layers(weights_by_policy[name]))
        critics.append(rllib_fcnet_value_layers(weights_by_policy[name]))
    return actors, critics


def rllib_per_slice_weights(actors, critics, policy_prefix: str = "intra_slice_sched_", prefix: str = "internal_model."):
    """The inverse of ``rllib_per_slice_layers``: ``{"{policy_prefix}{s}": state_dict}`` from S actor layer stacks and S critic
    layer stacks in slice order -- e.g. ``env.net_weights("intra", slice=s)`` / ``("v_intra", slice=s)`` after
    ``ppo_update_per_slice`` -- with a separate value branch (``vf_share_layers`` off), so that
    ``rllib_per_slice_layers(rllib_per_slice_weights(a, c), S)`` returns the same tensors.  The key names rest on RLlib's source as
    ``rllib_fcnet_layers`` assumes it: parity with RLlib itself is unpinned, no real checkpoint has been written or read."""
    if len(actors) != len(critics):
        raise ValueError(f"{len(actors)} actors and {len(critics)} critics: one pair per slice")
    out = {}
    for s, (actor, critic) in enumerate(zip(actors, critics)):
        if len(actor) < 2 or len(critic) < 2:
            raise ValueError("a FullyConnectedNetwork has at least one hidden layer in front of its logits / value head")
        sd = {}
        for body, head, layers in (("_hidden_layers", "_logits", actor), ("_value_branch_separate", "_value_branch", critic)):
            for i, (w, b) in enumerate(layers[:-1]):
                sd[f"{prefix}{body}.{i}._model.0.weight"], sd[f"{prefix}{body}.{i}._model.0.bias"] = torch.as_tensor(w).detach().clone(), torch.as_tensor(b).detach().clone()
            sd[f"{prefix}{head}._model.0.weight"], sd[f"{prefix}{head}._model.0.bias"] = torch.as_tensor(layers[-1][0]).detach().clone(), torch.as_tensor(layers[-1][1]).detach().clone()
        out[f"{policy_prefix}{s}"] = sd
    return out


def rllib_fcnet_value_layers(state_dict, prefix: str = "internal_model."):
    """The critic of an RLlib ``FullyConnectedNetwork`` as (W, b) layers from a torch state dict: with a separate value branch
    (``vf_share_layers`` off) ``{prefix}_value_branch_separate.{i}._model.0.{weight,bias}`` then
    ``{prefix}_value_branch._model.0.{weight,bias}``; with shared layers the actor's ``{prefix}_hidden_layers.{i}...`` then
    ``_value_branch``.  Strict like ``rllib_fcnet_layers``: any other key under ``prefix`` raises ValueError (``_logits`` belongs
    to the actor and is skipped), as do a missing head or incomplete layers.  The key names rest on RLlib's source as
    ``rllib_fcnet_layers`` assumes it; no real checkpoint has been read."""
    sep, hidden, head = {}, {}, {}
    for key, val in state_dict.items():
        if not key.startswith(prefix):
            continue
        parts = key[len(prefix):].split(".")
        if len(parts) == 5 and parts[0] in ("_hidden_layers", "_value_branch_separate") and parts[1].isdigit() \
                and parts[2:4] == ["_model", "0"] and parts[4] in ("weight", "bias"):
            (hidden if parts[0] == "_hidden_layers" else sep).setdefault(int(parts[1]), {})[parts[4]] = torch.as_tensor(val)
        elif len(parts) == 4 and parts[0] in ("_logits", "_value_branch") and parts[1:3] == ["_model", "0"] and parts[3] in ("weight", "bias"):
            if parts[0] == "_value_branch":
                head[parts[3]] = torch.as_tensor(val)
        else:
            raise ValueError(f"not a FullyConnectedNetwork key: {key!r}")
    body = sep if sep else hidden
    if not body or set(head) != {"weight", "bias"}:
        raise ValueError(f"no FullyConnectedNetwork value branch under {prefix!r}: layers {sorted(body)}, head {sorted(head)}")
    if sorted(body) != list(range(len(body))) or any(set(v) != {"weight", "bias"} for v in body.values()):
        raise ValueError(f"value layers under {prefix!r} are incomplete: {sorted(body)}")
    return [(body[i]["weight"], body[i]["bias"]) for i in range(len(body))] + [(head["weight"], head["bias"])]


def rllib_fcnet_layers(state_dict, prefix: str = "internal_model."):
    """The (W, b) layers of an RLlib ``FullyConnectedNetwork`` policy head from a torch state dict: keys
    ``{prefix}_hidden_layers.{i}._model.0.{weight,bias}`` then ``{prefix}_logits._model.0.{weight,bias}`` (the value branch,
    ``_value_branch*``, is not part of the actor and is skipped).  Any other key under ``prefix`` -- a free_log_std vector, a
    different model class -- raises ValueError, as do missing layers.  Keys outside ``prefix`` are ignored.  The activation
    is not in a state dict: RLlib's default ``fcnet_activation`` is "tanh"."""
    hidden, logits = {}, {}
    for key, val in state_dict.items():
        if not key.startswith(prefix):
            continue
        rest = key[len(prefix):]
        parts = rest.split(".")
        if parts[0].startswith("_value_branch"):
            continue
        if len(parts) == 5 and parts[0] == "_hidden_layers" and parts[1].isdigit() and parts[2:4] == ["_model", "0"] \
                and parts[4] in ("weight", "bias"):
            hidden.setdefault(int(parts[1]), {})[parts[4]] = torch.as_tensor(val)
        elif len(parts) == 4 and parts[0] == "_logits" and parts[1:3] == ["_model", "0"] and parts[3] in ("weight", "bias"):
            logits[parts[3]] = torch.as_tensor(val)
        else:
            raise ValueError(f"not a FullyConnectedNetwork key: {key!r}")
    if not hidden or set(logits) != {"weight", "bias"}:
        raise ValueError(f"no FullyConnectedNetwork under {prefix!r}: hidden layers {sorted(hidden)}, logits {sorted(logits)}")
    if sorted(hidden) != list(range(len(hidden))) or any(set(v) != {"weight", "bias"} for v in hidden.values()):
        raise ValueError(f"hidden layers under {prefix!r} are incomplete: {sorted(hidden)}")
    return [(hidden[i]["weight"], hidden[i]["bias"]) for i in range(len(hidden))] + [(logits["weight"], logits["bias"])]


# --------------------------------------------------------------------------------------------
# the learned baselines SchedTWC / SchedColORAN on the device (RANENV_POLICY_HEAD_NETWORK): the normative restatement and the
# SB3 state-dict readers.  stable-baselines3 is not part of the test environment: the key names and the forward are restated from
# SB3's documented module layout, parity with SB3 itself is UNPINNED.
# --------------------------------------------------------------------------------------------
HEAD_TAG = 0x48454100            # counter word c3 of the head policy's Philox draws: tag + position (include/ranenv.h)
LOG_STD_MIN, LOG_STD_MAX = -20.0, 2.0      # SAC's clamp of the actor's log_std output


def head_policy_noise(env_ids, episode, step, S: int, seed: int):
    """The head policy's draws z float64 [B, S]: Box-Muller of Philox words 0 / 1 at counter (env id, episode, step, HEAD_TAG + j),
    key = seed."""
    col = lambda a: np.asarray(torch.as_tensor(a).cpu().numpy(), dtype=np.int64).reshape(-1, 1)  # noqa: E731
    c3 = HEAD_TAG + np.arange(S, dtype=np.int64)[None, :]
    d = philox4x32_10(col(env_ids), col(episode), col(step), c3, int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF)
    u1 = (d[0].astype(np.float64) + 1.0) * 2.0 ** -32
    u2 = d[1].astype(np.float64) * 2.0 ** -32
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(6.283185307179586 * u2)


def head_policy_actions(head_obs, actor, dist: str = "gauss_clip", log_std=None, stochastic: bool = False, seed: int = 0,
                        activation: Optional[str] = None, env_ids=None, episode=None, step=None, precision: str = "f32"):
    """What the device computes under RANENV_POLICY_HEAD_NETWORK, in plain torch / numpy (the normative statement the GPU tests
    compare against; include/ranenv.h spells out the same rules).

    ``head_obs`` [B, 10*S]; ``actor`` as for ``batched_env.policy_net_layers``.  Forward in float32, epilogue in float64:
      "gauss_clip" (SB3 PPO): mean = net(obs) [S], ``log_std`` [S] the policy's parameter; a = mean, or when ``stochastic``
          mean + exp(log_std) * z; score = clamp(a, -1, 1);
      "gauss_tanh" (SB3 SAC): (mu | log_std) = net(obs) [2S], log_std clamped to [-20, 2]; a = mu, or mu + exp(log_std) * z;
          score = tanh(a);
      z = ``head_policy_noise`` at (env_ids + b, episode[b], step[b]).  Nothing is masked: the step applies the slice rules.
    ``precision`` "bf16": the actor as bound with ``precision="bf16"`` (``_mlp_forward``).
    Returns (scores float64 [B, S], a float64 [B, S] -- the unclamped / unsquashed action) as CPU tensors."""
    from .batched_env import policy_net_layers
    head_obs = torch.as_tensor(head_obs).detach().cpu().to(torch.float32)
    B, S = head_obs.shape[0], head_obs.shape[1] // 10
    if dist not in ("gauss_clip", "gauss_tanh"):
        raise ValueError("dist must be 'gauss_clip' or 'gauss_tanh'")
    if (dist == "gauss_clip") != (log_std is not None):
        raise ValueError("log_std is required for gauss_clip and must be None for gauss_tanh")
    if activation is None and not isinstance(actor, torch.nn.Module):
        activation = "tanh" if dist == "gauss_clip" else "relu"
    layers, act = policy_net_layers(actor, activation, 10 * S, S if dist == "gauss_clip" else 2 * S)
    out = _mlp_forward(head_obs, [(w.cpu(), b.cpu()) for w, b in layers], act, precision).to(torch.float64)
    if dist == "gauss_clip":
        a = out
        ls = torch.as_tensor(log_std).detach().cpu().to(torch.float32).to(torch.float64).reshape(1, S)
    else:
        a, ls = out[:, :S], out[:, S:].clamp(LOG_STD_MIN, LOG_STD_MAX)
    if stochastic:
        if env_ids is None or episode is None or step is None:
            raise ValueError("stochastic actions need env_ids, episode and step")
        a = a + torch.exp(ls) * torch.from_numpy(head_policy_noise(env_ids, episode, step, S, seed))
    scores = a.clamp(-1.0, 1.0) if dist == "gauss_clip" else torch.tanh(a)
    return scores, a


def head_policy_logp(log_std, z=None, B: Optional[int] = None):
    """The log-probability ``collect_head()`` records ("gauss_clip" only), restated in numpy float64: the sum over ALL positions
    j = 0..S-1, ascending, of ((-0.5 z_j) z_j - log_std_j) - 0.5 ln 2 pi -- no masked term -- rounded once to float32.
    ``log_std`` float32 [S]; ``z`` [B, S] the draws the actions used (None = the mode, z = 0: give ``B``).  Returns float32 [B]."""
    as_np = lambda a, dt: np.asarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a, dtype=dt)  # noqa: E731
    ls = as_np(log_std, np.float32).astype(np.float64).reshape(-1)
    zz = np.zeros((int(B), ls.shape[0])) if z is None else as_np(z, np.float64)
    lp = np.zeros(zz.shape[0], dtype=np.float64)
    for j in range(ls.shape[0]):                                # ascending positions, as the kernel sums them
        lp = lp + (((-0.5 * zz[:, j]) * zz[:, j] - ls[j]) - HALF_LN_2PI)
    return lp.astype(np.float32)


# --------------------------------------------------------------------------------------------
# Off-policy (SAC) collection: the sampler's index rule and the soft Bellman target, restated (include/ranenv.h)
# --------------------------------------------------------------------------------------------
SAC_TAG = 0x53414300             # counter word c3 of the target's Philox draws: tag + position


def replay_sample_index(n: int, seed: int, draw: int, written: int, capacity: int, B: int) -> np.ndarray:
    """The ring rows ``replay_sample()`` draws: int64 [n], row i = floor(u_i * N / 2^64) with N = min(written, capacity) * B and
    u_i = o1 << 32 | o0 of Philox-4x32-10(counter = (i lo, i hi, draw lo, draw hi), key = seed).  slot = index // B, env = index % B."""
    i = np.arange(int(n), dtype=np.uint64)
    d = philox4x32_10(i & np.uint64(0xFFFFFFFF), i >> np.uint64(32), int(draw) & 0xFFFFFFFF, (int(draw) >> 32) & 0xFFFFFFFF,
                      int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF)
    N = min(int(written), int(capacity)) * int(B)
    return np.array([((int(hi) << 32 | int(lo)) * N) >> 64 for lo, hi in zip(d[0], d[1])], dtype=np.int64)


def sac_target_noise(n: int, S: int, seed: int, draw: int) -> np.ndarray:
    """The target's draws z float64 [n, S]: Box-Muller of Philox words 0 / 1 at counter (row lo, row hi, draw lo, SAC_TAG + j),
    key = seed."""
    i = np.arange(int(n), dtype=np.uint64).reshape(-1, 1)
    c3 = SAC_TAG + np.arange(S, dtype=np.int64)[None, :]
    d = philox4x32_10(i & np.uint64(0xFFFFFFFF), i >> np.uint64(32), int(draw) & 0xFFFFFFFF, c3, int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF)
    u1 = (d[0].astype(np.float64) + 1.0) * 2.0 ** -32
    u2 = d[1].astype(np.float64) * 2.0 ** -32
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(6.283185307179586 * u2)


def sac_targets_torch(next_obs, reward, done, actor, q1, q2, gamma: float = 0.99, ent_coef: float = 0.0, stochastic: bool = True,
                      seed: int = 0, draw: int = 0, activation: Optional[str] = None, device=None):
    """What ``BatchedRanEnv.sac_targets`` computes, in plain torch / numpy (the normative statement; include/ranenv.h spells out the
    same rules): SB3 SAC's target  r + gamma (1 - d) (min(Q1', Q2')(s', a') - ent_coef log pi(a'|s'))  with a' ~ pi(.|s').

    ``next_obs`` [n, 10*S], ``reward`` [n], ``done`` [n]; ``actor`` -> (mu | log_std) [2S], ``q1`` / ``q2``: [obs | action] [11S] ->
    1, as for ``batched_env.policy_net_layers`` (lists of (W, b): ``activation`` default relu).  Forwards in float32 (on ``device``:
    default the CPU), epilogue in float64, every output rounded once to float32:
      ls = clamp(log_std, -20, 2); g = mu + exp(ls) z (z = ``sac_target_noise``, 0 in the mode); a = tanh(g); a32 = float32(a)
      logp = sum_j ((((-0.5 z) z - ls) - 0.5 ln 2 pi) - log((1 - a a) + 1e-6))   (the Gaussian's log-probability of g, SB3's epsilon)
      target = float32(reward + (0 if done else 1) (gamma (min(Q1, Q2)([next_obs | a32]) - ent_coef logp)))
    Returns a dict of CPU tensors: ``target`` [n], ``next_action`` [n, S], ``next_logp`` [n], ``q`` [n, 2] float32, and float64
    ``mu`` / ``log_std`` (clamped) / ``z`` / ``logp64`` for inspection."""
    from .batched_env import policy_net_layers
    dev = torch.device("cpu") if device is None else torch.device(device)
    x = torch.as_tensor(next_obs).detach().to(device=dev, dtype=torch.float32)
    n, S = x.shape[0], x.shape[1] // 10
    default = lambda net: activation if activation is not None or isinstance(net, torch.nn.Module) else "relu"  # noqa: E731
    nets = [policy_net_layers(net, default(net), k, o) for net, k, o in ((actor, 10 * S, 2 * S), (q1, 11 * S, 1), (q2, 11 * S, 1))]
    fwd = lambda inp, k: _mlp_forward(inp, [(w.to(dev), b.to(dev)) for w, b in nets[k][0]], nets[k][1])  # noqa: E731
    out = fwd(x, 0).to(torch.float64)
    mu, ls = out[:, :S], out[:, S:].clamp(LOG_STD_MIN, LOG_STD_MAX)
    z = torch.from_numpy(sac_target_noise(n, S, seed, draw)).to(dev) if stochastic else torch.zeros_like(mu)
    a = torch.tanh(mu + torch.exp(ls) * z)
    a32 = a.to(torch.float32)
    logp = torch.zeros(n, dtype=torch.float64, device=dev)
    for j in range(S):                                          # ascending positions, as the kernel sums them
        logp = logp + ((((-0.5 * z[:, j]) * z[:, j] - ls[:, j]) - HALF_LN_2PI) - torch.log((1.0 - a[:, j] * a[:, j]) + 1e-6))
    xa = torch.cat([x, a32], dim=1)
    q = torch.cat([fwd(xa, 1), fwd(xa, 2)], dim=1)
    qmin = torch.minimum(q[:, 0].to(torch.float64), q[:, 1].to(torch.float64))
    r = torch.as_tensor(reward).detach().to(device=dev, dtype=torch.float32).to(torch.float64)
    nd = torch.where(torch.as_tensor(done).detach().to(dev) != 0, 0.0, 1.0).to(torch.float64)
    target = (r + nd * (float(gamma) * (qmin - float(ent_coef) * logp))).to(torch.float32)
    cpu = lambda t: t.detach().cpu()  # noqa: E731
    return {"target": cpu(target), "next_action": cpu(a32), "next_logp": cpu(logp.to(torch.float32)), "q": cpu(q), "mu": cpu(mu), "log_std": cpu(ls),
            "z": cpu(z), "logp64": cpu(logp)}


# --------------------------------------------------------------------------------------------
# The SAC update (ranenv_sac_update, include/ranenv.h "SAC update"): the actor pass's draws and the torch-autograd statement of a step
# --------------------------------------------------------------------------------------------
SAC_ACTOR_TAG = 0x53415000       # counter word c3 of the actor pass's Philox draws: tag + position ("SAP\0"; the target's is SAC_TAG)
SAC_UPDATE_SLIPS = ("stale_critics", "larger_critic", "clamped_gradient", "coef_after_update", "target_noise_for_actor", "short_logp",
                    "action_columns_pad32", "polyak_live")


def _sac_noise(n: int, S: int, seed: int, draw: int, first_row: int, tag: int) -> np.ndarray:
    i = (np.arange(int(n), dtype=np.uint64) + np.uint64(int(first_row))).reshape(-1, 1)
    c3 = tag + np.arange(S, dtype=np.int64)[None, :]
    d = philox4x32_10(i & np.uint64(0xFFFFFFFF), i >> np.uint64(32), int(draw) & 0xFFFFFFFF, c3, int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF)
    u1 = (d[0].astype(np.float64) + 1.0) * 2.0 ** -32
    u2 = d[1].astype(np.float64) * 2.0 ** -32
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(6.283185307179586 * u2)


def sac_actor_noise(n: int, S: int, seed: int, draw: int, first_row: int = 0) -> np.ndarray:
    """The actor pass's draws z float64 [n, S] of ``sac_update``: row k is the global row i = ``first_row`` + k; Box-Muller of Philox
    words 0 / 1 at counter (i lo, i hi, draw lo, SAC_ACTOR_TAG + j), key = seed.  The target pass of the same step draws
    ``sac_target_noise`` at the same rows: counter word 3 is SAC_TAG + j there."""
    return _sac_noise(n, S, seed, draw, first_row, SAC_ACTOR_TAG)


def sac_update_reference(batch, actor, q1, q2, q1_target, q2_target, log_ent_coef, steps: int = 1, minibatch: int = 256, lr: float = 3e-4,
                         gamma: float = 0.99, tau: float = 0.005, seed: int = 0, draw: int = 0, first_row: int = 0, auto: bool = True,
                         target_entropy: Optional[float] = None, act_actor: str = "relu", act_critic: str = "relu", state: Optional[dict] = None,
                         dtype=torch.float64, slip: Optional[str] = None):
    """THE NORMATIVE STATEMENT of ``sac_update``, torch autograd on the CPU: ``steps`` gradient steps of SB3's ``SAC.train`` with its
    defaults.  ``dtype`` is the nets': their weights, forwards, gradients and Adam run in it (float64: the reference; float32: the
    yardstick, the device's own split), while the epilogues -- the squashed Gaussian, the target, the losses -- are float64 on the nets'
    outputs either way, as on the device and in ``sac_targets_torch``.  ``batch``: ``obs`` / ``action`` / ``reward`` / ``next_obs`` / ``done`` with at least ``steps *
    minibatch`` rows, step g takes rows [g n, (g + 1) n); the five nets lists of ``(W, b)`` (copied); ``log_ent_coef`` a float32 scalar.
    Per step, with alpha = exp(log_ent_coef) as the previous step left it:
      1. y = float32(reward + (1 - done) gamma (min(Q1', Q2')(next_obs, a') - alpha logp(a')))  under the actor and the TARGET critics,
         a' from ``sac_target_noise`` at the rows' global indices -- ``sac_targets_torch``'s rule
      2. L_Q = 0.5 (mean (Q1 - y)^2 + mean (Q2 - y)^2) on [obs | action]; Adam over both critics
      3. under the critics AS UPDATED: ls = clamp(log_std, -20, 2), a = tanh(mu + exp(ls) z) with z = ``sac_actor_noise``,
         L_pi = mean(alpha logp - torch.minimum(Q1, Q2)([obs | float32(a)])); Adam over the actor.  (torch.minimum halves the gradient
         at a tie, the device takes Q1: the tests' inputs have none.)
      4. ``auto``: L_alpha = -mean(log_ent_coef (logp + target_entropy)) with 3's logp detached; Adam on the scalar
      5. target <- (1 - tau) target + tau critic
    Adam is ``ppo_adam_reference`` without a clip, eps 1e-8, a state per tensor.  Returns {"actor", "q1", "q2", "q1_target",
    "q2_target": the new layers, "log_ent_coef", "state", "stats": float64 [steps, 8] as ``_lib.SAC_STATS``, "grad": the LAST step's
    {"actor", "q1", "q2": [(dW, db)], "log_ent_coef"}, "target": every step's y}.  ``slip``: a deliberately wrong variant
    (``SAC_UPDATE_SLIPS``), for the tests that show the tolerances bite."""
    assert slip is None or slip in SAC_UPDATE_SLIPS, slip
    leaf = lambda x: torch.as_tensor(x).detach().cpu().to(dtype).clone().requires_grad_(True)  # noqa: E731
    held = lambda net: [(torch.as_tensor(w).detach().cpu().to(dtype).clone(), torch.as_tensor(b).detach().cpu().to(dtype).clone()) for w, b in net]  # noqa: E731
    actor, q1, q2 = ([(leaf(w), leaf(b)) for w, b in net] for net in (actor, q1, q2))
    targets = [held(q1_target), held(q2_target)]
    lec = torch.as_tensor(log_ent_coef).detach().cpu().reshape(()).to(torch.float32).to(dtype).clone().requires_grad_(True)
    cpu = {k: torch.as_tensor(v).detach().cpu() for k, v in batch.items()}
    n, S = int(minibatch), cpu["action"].shape[1]
    te = -float(S) if target_entropy is None else float(target_entropy)
    state = {"actor": {}, "q1": {}, "q2": {}, "log_ent_coef": {}} if state is None else state
    flat = lambda net: [p for wb in net for p in wb]  # noqa: E731
    pairs = lambda fl: [(fl[2 * i].detach().clone(), fl[2 * i + 1].detach().clone()) for i in range(len(fl) // 2)]  # noqa: E731

    def forward(x, layers, act):
        x = x.to(dtype)
        for i, (w, b) in enumerate(layers):
            x = x @ w.T + b
            if i < len(layers) - 1:
                x = torch.tanh(x) if act == "tanh" else torch.relu(x)
        return x.to(torch.float64)

    def squashed(out, z, positions=None):
        mu, raw = out[:, :S], out[:, S:]
        ls = raw.clamp(LOG_STD_MIN, LOG_STD_MAX)
        if slip == "clamped_gradient":
            ls = raw + (ls - raw).detach()
        a = torch.tanh(mu + torch.exp(ls) * z)
        terms = (((-0.5 * z) * z - ls) - HALF_LN_2PI) - torch.log((1.0 - a * a) + 1e-6)
        return a, terms[:, :S if positions is None else positions].sum(dim=1)

    f32 = lambda t: t.to(torch.float32).to(torch.float64)  # noqa: E731
    stats, grads, ys = np.zeros((steps, 8)), None, []
    for g in range(steps):
        rows = slice(g * n, (g + 1) * n)
        obs, nxt = cpu["obs"][rows].to(torch.float32).to(torch.float64), cpu["next_obs"][rows].to(torch.float32).to(torch.float64)
        act, rew = f32(cpu["action"][rows]), f32(cpu["reward"][rows])
        nd = torch.where(cpu["done"][rows] != 0, 0.0, 1.0).to(torch.float64)
        z_t = torch.from_numpy(_sac_noise(n, S, seed, draw, first_row + g * n, SAC_TAG))
        z_a = z_t if slip == "target_noise_for_actor" else torch.from_numpy(sac_actor_noise(n, S, seed, draw, first_row + g * n))

        def coef_step(logp):
            loss = -(lec * (logp.detach() + te)).mean()
            g_ent = torch.autograd.grad(loss, [lec])
            with torch.no_grad():
                ppo_adam_reference([lec], list(g_ent), state["log_ent_coef"], lr, 0.0, (0.9, 0.999), 1e-8)
            return loss.detach(), g_ent[0].detach().clone()

        lec_used, early = lec.detach().clone(), None
        if slip == "coef_after_update" and auto:
            with torch.no_grad():
                _, lp0 = squashed(forward(obs, actor, act_actor), z_a)
            early = coef_step(lp0)
        alpha = torch.exp(lec.detach())
        with torch.no_grad():
            a_t, lp_t = squashed(forward(nxt, actor, act_actor), z_t)
            xa = torch.cat([nxt, f32(a_t)], dim=1)
            qt = torch.minimum(forward(xa, targets[0], act_critic)[:, 0], forward(xa, targets[1], act_critic)[:, 0])
            y = f32(rew + nd * (gamma * (qt - alpha * lp_t)))
        ys.append(y.clone())
        x = torch.cat([obs, act], dim=1)
        qv = [forward(x, q, act_critic)[:, 0] for q in (q1, q2)]
        loss_q = 0.5 * (((qv[0] - y) ** 2).mean() + ((qv[1] - y) ** 2).mean())
        g_q = torch.autograd.grad(loss_q, flat(q1) + flat(q2))
        stale = [[(w.detach().clone(), b.detach().clone()) for w, b in q] for q in (q1, q2)]
        with torch.no_grad():
            ppo_adam_reference(flat(q1), list(g_q[:len(flat(q1))]), state["q1"], lr, 0.0, (0.9, 0.999), 1e-8)
            ppo_adam_reference(flat(q2), list(g_q[len(flat(q1)):]), state["q2"], lr, 0.0, (0.9, 0.999), 1e-8)
        a, lp = squashed(forward(obs, actor, act_actor), z_a, S - 1 if slip == "short_logp" else None)
        a32 = a + (f32(a) - a).detach()
        if slip == "action_columns_pad32":       # d/da_j taken from input column pad32(10 S) + j of the padded row: action column P + j, or padding
            P = (10 * S + 31) // 32 * 32 - 10 * S
            moved = [a32[:, m].detach() + ((a32[:, m - P] - a32[:, m - P].detach()) if m >= P else 0.0) for m in range(S)]
            a32 = torch.stack(moved, dim=1)
        xa = torch.cat([obs, a32], dim=1)
        qa = [forward(xa, q, act_critic)[:, 0] for q in ((stale[0], stale[1]) if slip == "stale_critics" else (q1, q2))]
        qmin = torch.maximum(qa[0], qa[1]) if slip == "larger_critic" else torch.minimum(qa[0], qa[1])
        loss_pi = (alpha * lp - qmin).mean()
        g_pi = torch.autograd.grad(loss_pi, flat(actor))
        with torch.no_grad():
            ppo_adam_reference(flat(actor), list(g_pi), state["actor"], lr, 0.0, (0.9, 0.999), 1e-8)
        loss_ent, g_ent = torch.zeros((), dtype=torch.float64), torch.zeros((), dtype=torch.float64)
        if auto:
            loss_ent, g_ent = early if early is not None else coef_step(lp)
        with torch.no_grad():
            for tg, q in zip(targets, (q1, q2)):
                for (tw, tb), (w, b) in zip(tg, q):
                    if slip == "polyak_live":
                        w.copy_((1.0 - tau) * tw + tau * w)
                        b.copy_((1.0 - tau) * tb + tau * b)
                    else:
                        tw.copy_((1.0 - tau) * tw + tau * w)
                        tb.copy_((1.0 - tau) * tb + tau * b)
        stats[g] = [float(loss_q.detach()), float(loss_pi.detach()), float(loss_ent), float(torch.exp(lec_used)) if slip != "coef_after_update" else float(alpha),
                    float(lp.detach().mean()), float(qv[0].detach().mean()), float(qv[1].detach().mean()), float(y.mean())]
        nq = len(flat(q1))
        grads = {"actor": pairs(list(g_pi)), "q1": pairs(list(g_q[:nq])), "q2": pairs(list(g_q[nq:])), "log_ent_coef": g_ent}
    det = lambda net: [(w.detach(), b.detach()) for w, b in net]  # noqa: E731
    return {"actor": det(actor), "q1": det(q1), "q2": det(q2), "q1_target": targets[0], "q2_target": targets[1], "log_ent_coef": lec.detach(),
            "state": state, "stats": stats, "grad": grads, "target": torch.cat(ys)}


def sb3_sac_state_dict(actor_layers, q1, q2, q1_target, q2_target, log_ent_coef=None):
    """The inverse of ``sb3_sac_actor_layers`` plus the critics: an SB3 ``SAC`` ``MlpPolicy`` state dict from the stacked actor layers
    (``sac_net_weights("actor")``: the (mu | log_std) output layer is split into ``actor.mu`` / ``actor.log_std``), the live critics as
    ``critic.qf0`` / ``critic.qf1`` and the target critics as ``critic_target.qf0`` / ``critic_target.qf1`` (``create_mlp``
    Sequentials: Linear layers at the even indices), and, if given, ``log_ent_coef`` [1] (a parameter of SB3's algorithm object, not
    of its policy: returned under that name for the caller to place).  ``sb3_sac_actor_layers`` of the result returns the actor's
    tensors.  Key names restated from SB3's documented module layout: parity with SB3 itself is unpinned."""
    if len(actor_layers) < 2:
        raise ValueError("an SAC actor has at least one hidden layer in front of mu / log_std")
    t = lambda x: torch.as_tensor(x).detach().clone()  # noqa: E731
    out = {}
    for i, (w, b) in enumerate(actor_layers[:-1]):
        out[f"actor.latent_pi.{2 * i}.weight"], out[f"actor.latent_pi.{2 * i}.bias"] = t(w), t(b)
    w, b = actor_layers[-1]
    if w.shape[0] % 2:
        raise ValueError(f"the actor's output layer stacks (mu | log_std): {w.shape[0]} rows cannot be split")
    S = w.shape[0] // 2
    out["actor.mu.weight"], out["actor.mu.bias"] = t(w[:S]), t(b[:S])
    out["actor.log_std.weight"], out["actor.log_std.bias"] = t(w[S:]), t(b[S:])
    for prefix, nets in (("critic", (q1, q2)), ("critic_target", (q1_target, q2_target))):
        for k, net in enumerate(nets):
            for i, (w, b) in enumerate(net):
                out[f"{prefix}.qf{k}.{2 * i}.weight"], out[f"{prefix}.qf{k}.{2 * i}.bias"] = t(w), t(b)
    if log_ent_coef is not None:
        out["log_ent_coef"] = t(log_ent_coef).reshape(1)
    return out


def sb3_sac_critic_layers(state_dict, prefix: str = "critic"):
    """(q1, q2) of an SB3 ``SAC`` policy state dict: the ``{prefix}.qf0`` / ``{prefix}.qf1`` Sequentials (``prefix`` "critic" or
    "critic_target") as lists of (W, b) -- what ``set_sac_critics`` takes."""
    return tuple(_sb3_sequential(state_dict, f"{prefix}.qf{k}.", f"{prefix}.qf{k}") for k in (0, 1))


def _sb3_sequential(state_dict, prefix: str, what: str):
    """(W, b) of the Linear layers of an SB3 ``create_mlp`` Sequential under ``prefix`` (indices 0, 2, 4, ...: activations between)."""
    found = {}
    for key, val in state_dict.items():
        if not key.startswith(prefix):
            continue
        parts = key[len(prefix):].split(".")
        if len(parts) != 2 or not parts[0].isdigit() or int(parts[0]) % 2 or parts[1] not in ("weight", "bias"):
            raise ValueError(f"not a key of an SB3 MLP under {prefix!r}: {key!r}")
        found.setdefault(int(parts[0]) // 2, {})[parts[1]] = torch.as_tensor(val)
    if not found or sorted(found) != list(range(len(found))) or any(set(v) != {"weight", "bias"} for v in found.values()):
        raise ValueError(f"{what}: the layers under {prefix!r} are missing or incomplete: {sorted(found)}")
    return [(found[i]["weight"], found[i]["bias"]) for i in range(len(found))]


def _sb3_linear(state_dict, name: str):
    if f"{name}.weight" not in state_dict or f"{name}.bias" not in state_dict:
        raise ValueError(f"no {name}.weight / {name}.bias in the state dict")
    return torch.as_tensor(state_dict[f"{name}.weight"]), torch.as_tensor(state_dict[f"{name}.bias"])


def sb3_ppo_layers(state_dict):
    """An SB3 ``PPO`` ``MlpPolicy`` (``ActorCriticPolicy``, separate ``net_arch`` for pi and vf) from ``policy.state_dict()``:
    returns (actor layers, log_std [S], critic layers) with actor = ``mlp_extractor.policy_net.{0,2,..}`` then ``action_net``,
    critic = ``mlp_extractor.value_net.{0,2,..}`` then ``value_net``, and the ``log_std`` parameter.  Any other key (a features
    extractor with weights, a shared trunk) raises ValueError, as do missing ones.  The activation is not in a state dict: SB3's
    default is tanh.  Key names restated from SB3's documented module layout: no real checkpoint has been read."""
    known = ("mlp_extractor.policy_net.", "mlp_extractor.value_net.", "action_net.", "value_net.")
    for key in state_dict:
        if key != "log_std" and not key.startswith(known):
            raise ValueError(f"not a key of an SB3 PPO MlpPolicy: {key!r}")
    if "log_std" not in state_dict:
        raise ValueError("no log_std in the state dict (a PPO policy for a Box action space has one)")
    actor = _sb3_sequential(state_dict, "mlp_extractor.policy_net.", "actor") + [_sb3_linear(state_dict, "action_net")]
    critic = _sb3_sequential(state_dict, "mlp_extractor.value_net.", "critic") + [_sb3_linear(state_dict, "value_net")]
    return actor, torch.as_tensor(state_dict["log_std"]), critic


def sb3_sac_actor_layers(state_dict):
    """The actor of an SB3 ``SAC`` ``MlpPolicy`` from ``policy.state_dict()``: ``actor.latent_pi.{0,2,..}`` then the ``actor.mu``
    and ``actor.log_std`` Linear layers STACKED into one output layer (mu | log_std), the form "gauss_tanh" takes.  Keys outside
    ``actor.`` (the critics, their targets) are ignored; any other key under ``actor.`` raises ValueError, as do missing ones.
    SB3's default activation for SAC is relu.  Key names restated from SB3's documented module layout."""
    for key in state_dict:
        if key.startswith("actor.") and not key.startswith(("actor.latent_pi.", "actor.mu.", "actor.log_std.")):
            raise ValueError(f"not a key of an SB3 SAC actor: {key!r}")
    body = _sb3_sequential(state_dict, "actor.latent_pi.", "actor")
    (wm, bm), (wl, bl) = _sb3_linear(state_dict, "actor.mu"), _sb3_linear(state_dict, "actor.log_std")
    if wm.shape != wl.shape:
        raise ValueError(f"actor.mu {tuple(wm.shape)} and actor.log_std {tuple(wl.shape)} differ in shape")
    return body + [(torch.cat([wm, wl], dim=0), torch.cat([bm, bl], dim=0))]
