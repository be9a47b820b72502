"""The head policy source "inter" (ranenv_set_head_policy_source: the reference's IBSchedSB3, agents/sb3_sched.py) as far as it shows
without a GPU: the new symbol in header, library and binding, InterVecEnv's spaces, and the Python argument rules."""
from __future__ import annotations

import ctypes
import os
import re
import types

import pytest

torch = pytest.importorskip("torch")

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_library_exports_the_source_call():
    from intent_radio_sched_multi_slice_amd import _lib
    from intent_radio_sched_multi_slice_amd.csrc import build
    build.build()
    header = open(os.path.join(REPO, "include", "ranenv.h")).read()
    assert re.search(r"\bint\s+ranenv_set_head_policy_source\s*\(\s*ranenv_handle\s+h\s*,\s*int32_t\s+source\s*\)\s*;", header)
    values = dict(re.findall(r"#define\s+(RANENV_HEAD_SRC_[A-Z]+)\s+(\d+)", header))
    assert values == {"RANENV_HEAD_SRC_HEAD": "0", "RANENV_HEAD_SRC_INTER": "1"}
    assert (_lib.HEAD_SRC_HEAD, _lib.HEAD_SRC_INTER) == (0, 1)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(raw, "ranenv_set_head_policy_source")
    # the two lines that counted sb3_sched.py among the readers of the head observation are gone
    assert not re.search(r"sb3_sched\.py\)\s+that read the head observation", header)


def test_binding_has_the_prototype():
    from intent_radio_sched_multi_slice_amd import _lib
    restype, argtypes = _lib.FUNCTIONS["ranenv_set_head_policy_source"]
    assert restype is ctypes.c_int and argtypes == [ctypes.c_void_p, ctypes.c_int32]
    assert "ranenv_set_head_policy_source" in _lib.EXPORTS
    fn = _lib.load().ranenv_set_head_policy_source
    assert fn.argtypes == [ctypes.c_void_p, ctypes.c_int32]
    assert fn(None, 0) == -1                                   # RANENV_E_INVALID: a null handle, no device touched


def _stub_env(S=5, Us=10, B=4):
    calls = []
    env = types.SimpleNamespace(B=B, S=S, Us=Us, device=torch.device("cpu"), set_policy=lambda *a: calls.append(a))
    return env, calls


@pytest.mark.parametrize("S,Us", [(5, 10), (10, 10)])
def test_inter_vec_env_spaces_are_player_0s(S, Us):
    from intent_radio_sched_multi_slice_amd import _lib, adapters
    env, calls = _stub_env(S, Us)
    marl = adapters.MarlBatchEnv(env)
    want_obs = adapters.describe_space(marl.observation_space["player_0"])["observations"]
    want_act = adapters.describe_space(marl.action_space["player_0"])
    for intra, code in (("rr", _lib.INTRA_RR), ("pf", _lib.INTRA_PF)):
        venv = adapters.InterVecEnv(env, intra=intra)
        assert adapters.describe_space(venv.observation_space) == want_obs
        assert adapters.describe_space(venv.action_space) == want_act
        assert want_obs["shape"] == [10 * S] and want_act == {"shape": [S], "low": -1.0, "high": 1.0, "dtype": "float64"}
        assert venv.num_envs == env.B and calls[-1] == (_lib.POLICY_EXTERNAL, code)
        assert type(venv).__mro__[1] is adapters.HeadVecEnv.__mro__[1]        # beside HeadVecEnv, on the same base
    with pytest.raises(ValueError):
        adapters.InterVecEnv(env, intra="mt")


def test_argument_rules_raise_before_the_device():
    from intent_radio_sched_multi_slice_amd import batched_env as be
    # reward names per source
    assert be.head_reward_column("head", "twc") == 0 and be.head_reward_column("head", "colran") == 1
    assert be.head_reward_column("inter", "ibsched") == 0
    assert be.head_reward_column("head") == 0 and be.head_reward_column("inter") == 0
    for source, name in (("inter", "twc"), ("inter", "colran"), ("head", "ibsched"), ("head", "other"), ("both", "twc")):
        with pytest.raises(ValueError):
            be.head_reward_column(source, name)
    # the methods apply them to the source in force, ahead of every library call (the stub has no handle and no library)
    for source, bad in (("inter", "twc"), ("inter", "colran"), ("head", "ibsched")):
        stub = types.SimpleNamespace(_recorder=None, head_observation=source)
        with pytest.raises(ValueError):
            be.BatchedRanEnv.collect_head(stub, 4, reward=bad)
        with pytest.raises(ValueError):
            be.BatchedRanEnv.replay_sample(stub, 4, reward=bad)
    # an unknown observation
    stub = types.SimpleNamespace(head_observation="head", head_obs=None, tables=None)
    with pytest.raises(ValueError, match="observation"):
        be.BatchedRanEnv.set_head_policy_network(stub, None, observation="both")
    # "head" still needs enable_heads(); "inter" does not get that far without a library, but it is not refused for head_obs
    with pytest.raises(be.RanEnvError, match="enable_heads"):
        be.BatchedRanEnv.set_head_policy_network(stub, None, "gauss_clip", torch.zeros(5), observation="head")
    assert set(be.HEAD_SOURCES) == {"head", "inter"}
