"""One SHA-256 per case over everything a PPO update writes that the facade reads back -- weights, both moments and the step counters
of every bound net, log_std and its moments, dev_grad, the statistics -- for every PPO training kernel, on the smallest cases at which
a tile function can go wrong.  The cases and their fixtures are the GPU tests' own (tests/ppo_update_ref.py, ppo_mixed_ref.py,
ppo_wide_ref.py, ppo_head_ref.py, ppo_spread_ref.py and the helpers of tests/test_gpu_ppo_*.py).  The package loads whichever library
RANENV_LIB names, so two builds are compared by running this once under each, each in a process of its own:

    RANENV_LIB=parent.so python tools/ppo_update_digest.py --out parent.json
    python tools/ppo_update_digest.py --out new.json
    python tools/ppo_update_digest.py --join parent.json new.json --out profiles/ppo_refactor_digests.json     # exit 1 where a digest differs

A change that only moves the training kernels' text leaves every digest as it was: -ffp-contract=off and an unchanged expression order
leave no room for a last-bit difference."""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

TRAIN = dict(lr=2e-3, clip=0.2, vf_coeff=0.5, ent_coeff=0.01, grad_clip=0.5)      # adv_norm: the facade's default, "minibatch"


def digest(*parts):
    """SHA-256 over dicts of arrays (numpy or torch, device or host): every entry's name, dtype, shape and bytes, names in order"""
    import numpy as np
    import torch
    h = hashlib.sha256()
    for i, d in enumerate(parts):
        for k in sorted(d):
            x = d[k].detach().cpu().numpy() if isinstance(d[k], torch.Tensor) else np.asarray(d[k])
            h.update(f"{i}/{k}/{x.dtype}/{x.shape}/".encode())
            h.update(np.ascontiguousarray(x).tobytes())
    return h.hexdigest()


def cases():
    """(name, digest) of every case, in a fixed order"""
    import numpy as np
    import torch
    from tests import ppo_head_ref as hd
    from tests import ppo_mixed_ref as mx
    from tests import ppo_update_ref as ref
    from tests import ppo_wide_ref as wd
    from tests import test_gpu_ppo_head as t_head
    from tests import test_gpu_ppo_head_spread as t_hs
    from tests import test_gpu_ppo_mixed as t_mixed
    from tests import test_gpu_ppo_per_slice as t_ps
    from tests import test_gpu_ppo_spread as t_spread
    from tests import test_gpu_ppo_update as t_up
    from tests import test_gpu_ppo_wide as t_wide
    G = len(ref.FIRST) - 1

    # ---- the body kernel: ref.CASES, members of 16 / 32 / 48 inter rows, critics of both kinds, minibatch 12, 2 epochs -----------------
    for case in ref.CASES:
        env, _ = t_up._env(case)
        rec = t_up._record(env)
        order = t_up._order(rec, ref.FIRST, 2)
        out = env.ppo_update(rec, epochs=2, minibatch=ref.MINIBATCH, order=order, grad=True, **TRAIN)
        yield f"body/{case}", digest(ref.state(env, G), out)
        if case == "tanh40x24":          # ... and once a list with an entry of -1 and one beyond the record, per member and kind
            T, B, S = rec["mask_inter"].shape
            bad = {k: order[k].clone() if isinstance(order[k], torch.Tensor) else order[k] for k in order}
            for kind, n_record in (("inter", T * B), ("intra", T * B * S)):
                f = bad["first_" + kind]
                for m in range(G):
                    bad["order_" + kind][:, int(f[m]) + 1], bad["order_" + kind][:, int(f[m + 1]) - 1] = -1, n_record + 7
            out = env.ppo_update(rec, epochs=2, minibatch=ref.MINIBATCH, order=bad, grad=True, **TRAIN)
            yield f"body/{case}/entries outside the record", digest(ref.state(env, G), out)
        env.close()

    # ---- mixed: the three-member cases of tests/test_gpu_ppo_mixed.py ------------------------------------------------------------------
    for case in mx.CASES:
        env, out, _ = t_mixed._mixed_run(case)
        yield f"mixed/{case}", digest(ref.state(env, t_mixed.G3), out)
        env.close()

    # ---- wide and mixed-wide: where both plans hold, and [512] x 3 on a single minibatch -------------------------------------------------
    env = t_wide._both_plans_env("tanh40x24", True)
    rec = env.collect(ref.T)
    out = env.ppo_update(rec, epochs=2, minibatch=ref.MINIBATCH, order=t_wide._order(rec, ref.FIRST, 2), grad=True, **TRAIN)
    yield "wide/tanh40x24", digest(ref.state(env, G), out)
    env.close()
    env = t_wide._beyond_env("verybig")
    rec = t_wide._on_device(env, wd.beyond_record("verybig"))
    out = env.ppo_update(rec, epochs=1, minibatch=ref.ALL, order=t_wide._on_device(env, wd.order(wd.beyond_record("verybig"), 1)), grad=True, **TRAIN)
    yield "wide/verybig, one minibatch", digest(ref.state(env, G), out)
    env.close()
    small = [wd.MIXED[0], ([24], "relu"), wd.MIXED[2]]
    for name, shapes, hp in (("both plans", small, dict(epochs=2, minibatch=ref.MINIBATCH)), ("verybig member, one minibatch", wd.MIXED, dict(epochs=1, minibatch=ref.ALL))):
        env = t_wide._population_env(wd.mixed_nets(shapes), True, True)
        rec = t_wide._on_device(env, wd.mixed_record())
        out = env.ppo_update(rec, order=t_wide._on_device(env, wd.order(wd.mixed_record(), hp["epochs"])), grad=True, **hp, **TRAIN)
        yield f"mixed_wide/{name}", digest(ref.state(env, G), out)
        env.close()

    # ---- per slice, plain and wide: the cases of tests/test_gpu_ppo_per_slice.py, one empty slice once -----------------------------------
    for bind in (dict(), dict(wide=True)):
        for case, empty in [(c, None) for c in ref.CASES] + [("tanh40x24", 1)]:
            run = t_ps._run(case, empty=empty, **bind)
            name = f"per_slice{'_wide' if bind else ''}/{case}" + ("" if empty is None else f"/slice {empty} empty")
            yield name, digest(run["out"], run["inter"], *run["slices"])

    # ---- head: hd.CASES (S 1, 3, 5, 16) on the 96-row record, minibatch 12, 2 epochs ---------------------------------------------------------
    for case in hd.CASES:
        env, _, rec = t_head._case_env(case)
        out = env.ppo_update_head(rec, epochs=2, minibatch=hd.MINIBATCH, order=t_head._dev(hd.row_order(2), env), grad=True, **t_head.TRAIN)
        yield f"head/{case}", digest(hd.head_state(env), out)
        env.close()

    # ---- spread and head-spread: 1 and 3 slabs, 65 rows at minibatch 40 (a two-tile step and a one-tile tail step), 2 epochs -------------
    for bind in (dict(slabs=1), dict(slabs=3), dict(slabs=3, wide=True)):
        env = t_spread._env("tanh40x24", spread=True, **bind)
        rec = env.collect(ref.T)
        order = t_spread._order(rec, 2)
        for kind in ("inter", "intra"):
            order["order_" + kind], order["first_" + kind] = order["order_" + kind][:2, :65].contiguous(), np.array([0, 65], dtype=np.int32)
        out = env.ppo_update(rec, epochs=2, minibatch=40, order=order, grad=True, **TRAIN)
        yield f"spread/{bind['slabs']} slabs" + (", wide" if "wide" in bind else ""), digest(ref.state(env, 1), out)
        env.close()
    for slabs in (1, 3):
        env, _, rec = t_hs._env("base", slabs)
        order = hd.row_order(2)[:, :65].contiguous()
        out = env.ppo_update_head(rec, epochs=2, minibatch=40, order=t_hs._dev(order, env), grad=True, **t_hs.TRAIN)
        yield f"head_spread/{slabs} slabs", digest(hd.head_state(env), out)
        env.close()


def join(a_path, b_path, out):
    with open(a_path) as f:
        a = json.load(f)
    with open(b_path) as f:
        b = json.load(f)
    names = list(a["digests"])
    assert names == list(b["digests"]), "the two runs hold different cases"
    differ = [n for n in names if a["digests"][n] != b["digests"][n]]
    result = {"libraries": [a["library"], b["library"]], "cases": {n: [a["digests"][n], b["digests"][n]] for n in names}, "differ": differ}
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
    print(f"{len(names)} cases, {len(differ)} differ" + "".join(f"\n  DIFFERS: {n}" for n in differ))
    return 1 if differ else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--join", nargs=2, metavar=("A.json", "B.json"), default=None)
    args = ap.parse_args()
    if args.join:
        sys.exit(join(args.join[0], args.join[1], args.out or os.path.join(REPO, "profiles", "ppo_refactor_digests.json")))
    t0 = time.perf_counter()
    result = {"library": os.path.basename(os.environ.get("RANENV_LIB", "")) or "the tree's own", "digests": {}}
    for name, d in cases():
        result["digests"][name] = d
        print(f"{d}  {name}", flush=True)
    print(f"{len(result['digests'])} cases in {time.perf_counter() - t0:.1f} s", flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
