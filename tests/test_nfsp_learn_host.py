"""CPU checks of the fused learner's two host-side pieces: the NumPy float64 restatement (tests/nfsp_learn_cases.py)
against torch float64 autograd, and the LDS planner (csrc/osg_mlp_plan.h) through a small stand-alone program."""
import os
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import nfsp_learn_cases as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_LIMIT = 160 * 1024


@pytest.mark.parametrize("kind", [0, 1])
def test_the_restatement_steps_by_torch_float64_gradients(kind):
    rng = np.random.default_rng(7 + kind)
    widths, I, B, lr = [6, 5, 4, 3], 9, 7, 0.1
    n = sum(o * i + o for i, o in zip(widths[:-1], widths[1:]))
    params, target = rng.normal(0, 0.5, n), rng.normal(0, 0.5, n)
    tensors = rng.normal(0, 1, (I, widths[0]))
    mask = rng.random((I, 3)) < 0.7
    mask[:, 0] = True
    mask[0, 1:] = False                                        # a single legal action
    info = rng.integers(0, I, (1, B))
    info[0, 0] = 0
    if kind == 0:
        rows = (info, rng.integers(0, 3, (1, B)), rng.normal(0, 1, (1, B)), rng.integers(0, I, (1, B)), (rng.random((1, B)) < 0.4).astype(np.uint8))
        kw = dict(discount=0.9, loss="huber", beta=0.5)
    else:
        probs = rng.random((1, B, 3)) * mask[info]
        rows = (info, probs / probs.sum(-1, keepdims=True))
        kw = dict(clip=0.05)
    got, loss, margin = lc.learn(kind, widths, params, target, tensors, mask, rows, lr, **kw)
    assert margin > 1e-9

    t = [torch.tensor(a, dtype=torch.float64) for a in (params, target, tensors)]
    t[0].requires_grad_(True)

    def net(flat, x):
        layers = lc.unflatten(flat, widths)
        for k, (w, b) in enumerate(layers):
            x = x @ w.T + b
            x = torch.relu(x) if k + 1 < len(layers) else x
        return x
    m = torch.tensor(mask)
    y = net(t[0], t[2][info[0]])
    if kind == 0:
        live = torch.tensor(rows[4][0] == 0)
        nq = net(t[1], t[2][rows[3][0]] * live[:, None]).masked_fill(~(m[rows[3][0]] & live[:, None]), torch.finfo(torch.float64).min).max(1)[0]
        tgt = (torch.tensor(rows[2][0]) + live.double() * 0.9 * nq).detach()
        out = F.smooth_l1_loss(y.gather(1, torch.tensor(rows[1][0])[:, None])[:, 0], tgt, beta=0.5)
    else:
        out = F.cross_entropy(torch.where(m[info[0]], y, torch.full_like(y, torch.finfo(torch.float32).min)), torch.tensor(rows[1][0]))
    out.backward()
    if kind == 1:
        torch.nn.utils.clip_grad_norm_([t[0]], 0.05)
    want = (t[0] - lr * t[0].grad).detach().numpy()
    assert abs(out.item() - loss[0]) < 1e-12
    assert np.abs(got - want).max() < 1e-12 and np.abs(got - params).max() > 1e-4


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mlp_plan") / "mlp_plan_host_test")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover",
                           "-I", os.path.join(ROOT, "open_spiel_amd", "csrc"), os.path.join(ROOT, "tests", "native", "mlp_plan_host_test.cpp"), "-o", exe])

    def run(widths, batch, dqn, limit=LDS_LIMIT):
        out = subprocess.check_output([exe, str(len(widths) - 1), *map(str, widths), str(batch), str(int(dqn)), str(limit)], text=True)
        return [line.split() for line in out.splitlines()]
    return run


def test_the_plan_fits_the_example_refuses_beyond_the_limit_and_pads_as_documented(plan):
    for dqn in (False, True):
        lines = plan([30, 128, 3], 128, dqn)
        assert lines[0][0] == "ok" and int(lines[0][1]) <= LDS_LIMIT and lines[0][2:] == ["128", str(128 * 30 + 128 + 3 * 128 + 3)]
        assert [l[1:] for l in lines if l[0] == "w"] == [["32", "128", "36", "0"], ["128", "16", "132", "20"]]
        assert [l[1] for l in lines if l[0] == "act"] == ["36", "132", "20"]
    for widths, batch in (([11, 8, 2], 1), ([17, 48, 2], 40), ([30, 32, 16, 3], 40), ([256, 32, 16], 16)):
        lines = plan(widths, batch, True)
        assert lines[0][0] == "ok"
        strides = [int(x) for l in lines[1:] for x in (l[3:] if l[0] == "w" else l[1:]) if int(x)]
        assert strides and all(s % 16 == 4 for s in strides)      # 4 mod 16: the bank argument of osg_mlp_plan.h
    need = int(plan([30, 128, 3], 128, True)[0][1])
    assert plan([30, 128, 3], 128, True, need)[0][0] == "ok"
    assert plan([30, 128, 3], 128, True, need - 1)[0][0] == "refused"
    assert plan([256, 128, 128, 16], 128, True)[0][0] == "refused"    # the widest served shape does not fit 160 KB
    for widths, batch in (([30, 129, 3], 8), ([257, 8, 3], 8), ([30, 8, 17], 8), ([30, 8, 3], 129), ([30, 8, 3], 0)):
        assert plan(widths, batch, False)[0][0] == "refused"
