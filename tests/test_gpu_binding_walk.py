"""Which net serves each of the four IBSched roles after every binding call (include/ranenv.h "Policy networks", "Populations"): a
walk through the binding calls that only binds and asks -- no step, no rollout.  A role (0 inter actor, 1 intra actor, 2 inter
critic, 3 intra critic) is served by its population nets, else its nets per slice, else its one net, and every binding call switches
forms of other roles off beside the ones it binds; the walk pins those rules, the asymmetric ones included (a plain policy bind
drops the population's critics, a population's policy bind leaves one-net critics standing).

The smallest shape with every form: 4 envs, S = 3, Us = 4, two members of two envs.  One hidden layer everywhere, whose width names
the form: ranenv_get_net_weights reports unpadded widths."""
from __future__ import annotations

import ctypes as C
import re

import pytest

torch = pytest.importorskip("torch")

from tests.gpu_common import make_inter_net, make_net, need_gpu

pytestmark = pytest.mark.gpu

E_INVALID, E_STATE = -1, -3
B, S, US = 4, 3, 4
FIRST = [0, 2, 4]
G = len(FIRST) - 1
ONE, SLICE, POP = 8, 16, 24          # the forms' hidden widths
IN_INTER, IN_INTRA = 10 * S, 2 * US + 9
NONE = None


def _structs(env, nets, in_dim, out_dim, keep):
    from intent_radio_sched_multi_slice_amd.batched_env import NET_INPUTS, policy_net_layers
    out = []
    for net in nets:
        layers, act = policy_net_layers(net, None, in_dim, out_dim)
        out.append(env._mlp_struct(layers, act, NET_INPUTS["obs"], keep))
    keep += out
    return out


def _array(structs):
    return (C.POINTER(type(structs[0])) * len(structs))(*[C.pointer(m) for m in structs])


class _Walk:
    def __init__(self, env):
        from intent_radio_sched_multi_slice_amd import _lib
        self.env, self.lib, self.h, self.Mlp = env, env._lib, env._h, _lib.Mlp

    def error(self):
        return (self.lib.ranenv_last_error(self.h) or b"").decode()

    def ask(self, role, member=0):
        """(status, hidden width or the error's text) of ranenv_get_net_weights with no buffers: nothing is copied"""
        out = self.Mlp()
        rc = self.lib.ranenv_get_net_weights(self.h, role, member, C.byref(out), self.env._stream())
        return (rc, out.dims[1]) if rc == 0 else (rc, self.error())

    def check(self, step, want):
        """``want`` [4]: per role ONE / SLICE / POP (the form that serves it, by its width) or NONE"""
        n = C.c_int32()
        assert self.lib.ranenv_get_population(self.h, C.byref(n), None) == 0
        for role, form in enumerate(want):
            tag = (step, "role", role)
            rc, got = self.ask(role)
            if form is NONE:
                assert rc == E_STATE and re.search(r"no .* net bound", got), (tag, rc, got)
            elif form == SLICE:
                assert rc == E_STATE and "bound per slice" in got, (tag, rc, got)
            else:
                assert (rc, got) == (0, form), (tag, rc, got)
            # member 1: served exactly where the population's nets are; a one net has member 0 alone
            rc, got = self.ask(role, 1)
            if form == POP:
                assert (rc, got) == (0, POP), (tag, "member 1", rc, got)
            else:
                assert rc == (E_INVALID if form == ONE else E_STATE), (tag, "member 1", rc, got)
            # ... and the population's own getter (member 1 exists only under a grouping: without one the member check refuses first)
            rc = self.lib.ranenv_get_population_net(self.h, role, 1, None, None, None, None, None)
            assert rc == (E_INVALID if n.value == 0 else (0 if form == POP else E_STATE)), (tag, "ranenv_get_population_net", rc, self.error())


def test_every_binding_call_leaves_each_role_with_the_form_the_rules_say():
    need_gpu()
    from intent_radio_sched_multi_slice_amd.batched_env import BatchedRanEnv
    env = BatchedRanEnv(batch=B, n_slices=S, n_ues=S * US, n_rbs=25, max_ues_slice=US)
    w = _Walk(env)
    lib, h, st, keep = w.lib, w.h, env._stream(), []
    inter = lambda width, seed: make_inter_net(S, [width], "tanh", seed)                                   # noqa: E731
    intra = lambda width, out, seed: make_net([IN_INTRA, width, out], "tanh", seed)                         # noqa: E731
    v_inter = lambda width, seed: make_net([IN_INTER, width, 1], "tanh", seed)                              # noqa: E731
    one_a, = _structs(env, [inter(ONE, 1)], IN_INTER, 2 * S, keep)
    one_i, = _structs(env, [intra(ONE, 3, 2)], IN_INTRA, 3, keep)
    one_v, = _structs(env, [v_inter(ONE, 3)], IN_INTER, 1, keep)
    one_vi, = _structs(env, [intra(ONE, 1, 4)], IN_INTRA, 1, keep)
    ps_i = _array(_structs(env, [intra(SLICE, 3, 10 + s) for s in range(S)], IN_INTRA, 3, keep))
    ps_vi = _array(_structs(env, [intra(SLICE, 1, 20 + s) for s in range(S)], IN_INTRA, 1, keep))
    pop_a = _array(_structs(env, [inter(POP, 30 + m) for m in range(G)], IN_INTER, 2 * S, keep))
    pop_i = _array(_structs(env, [intra(POP, 3, 40 + m) for m in range(G)], IN_INTRA, 3, keep))
    pop_v = _array(_structs(env, [v_inter(POP, 50 + m) for m in range(G)], IN_INTER, 1, keep))
    pop_vi = _array(_structs(env, [intra(POP, 1, 60 + m) for m in range(G)], IN_INTRA, 1, keep))
    first = (C.c_int32 * len(FIRST))(*FIRST)
    ok = lambda rc: (rc, w.error() if rc else "")                                                           # noqa: E731

    w.check(1, [NONE, NONE, NONE, NONE])
    assert ok(lib.ranenv_set_policy_network(h, C.byref(one_a), C.byref(one_i), 1, 7, st)) == (0, "")
    w.check(2, [ONE, ONE, NONE, NONE])
    assert ok(lib.ranenv_set_value_network(h, C.byref(one_v), C.byref(one_vi), st)) == (0, "")
    w.check(3, [ONE, ONE, ONE, ONE])
    assert ok(lib.ranenv_set_intra_policy_networks(h, S, ps_i, st)) == (0, "")
    w.check(4, [ONE, SLICE, ONE, ONE])
    assert ok(lib.ranenv_set_intra_value_networks(h, S, ps_vi, st)) == (0, "")
    w.check(5, [ONE, SLICE, ONE, SLICE])
    assert ok(lib.ranenv_set_intra_policy_networks(h, 0, None, st)) == (0, "")      # drops the critics per slice with the actors
    w.check(6, [ONE, ONE, ONE, ONE])
    assert ok(lib.ranenv_set_population(h, G, first)) == (0, "")
    assert ok(lib.ranenv_set_population_value(h, G, pop_v, None, st)) == (0, "")    # intra NULL: no intra critic now
    w.check(7, [ONE, ONE, POP, NONE])
    assert ok(lib.ranenv_set_value_network(h, C.byref(one_v), C.byref(one_vi), st)) == (0, "")
    w.check(8, [ONE, ONE, ONE, ONE])
    assert ok(lib.ranenv_set_population_policy(h, G, pop_a, pop_i, 1, 7, st)) == (0, "")      # one-net critics stay
    w.check(9, [POP, POP, ONE, ONE])
    assert lib.ranenv_ppo_bind(h, st) == E_STATE and "every net per member or every net single" in w.error()
    assert ok(lib.ranenv_set_population_value(h, G, pop_v, pop_vi, st)) == (0, "")
    w.check(10, [POP, POP, POP, POP])
    assert ok(lib.ranenv_ppo_bind(h, st)) == (0, "")
    assert ok(lib.ranenv_ppo_state(h, 0, 1, None, None, None, None)) == (0, "")
    assert ok(lib.ranenv_set_policy_network(h, C.byref(one_a), None, 1, 7, st)) == (0, "")    # no population acts or values now
    w.check(11, [ONE, NONE, NONE, NONE])
    n, got = C.c_int32(), (C.c_int32 * (G + 1))()
    assert lib.ranenv_get_population(h, C.byref(n), got) == 0 and (n.value, list(got)) == (G, FIRST)
    assert lib.ranenv_ppo_state(h, 0, 0, None, None, None, None) == E_STATE      # the PPO binding ended with its nets
    assert ok(lib.ranenv_set_population(h, 0, None)) == (0, "")
    w.check(12, [ONE, NONE, NONE, NONE])
    torch.cuda.synchronize()
    env.close()
