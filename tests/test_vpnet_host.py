"""CPU checks of the fused policy-value forward's planner (csrc/osg_vpnet_plan.h) through a small stand-alone program, and
of alpha_zero.VPNetMLP against a float64 NumPy restatement of alpha_zero_torch/model.cc:216-263, 318-376, 391-396."""
import os
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_LIMIT = 160 * 1024


def reference_forward(flat, shape, obs, legal):
    """The network in float64: (prior [n, A] — softmax over the legal actions, 0 elsewhere and in a row without one —,
    value [n]).  flat: the parameters in the ABI's order; shape: (O, W, depth, A)."""
    O, W, D, A = shape
    flat, at, layers = np.asarray(flat, np.float64), 0, []
    for o, i in [(W, O)] + [(W, W)] * D + [(W, W), (1, W), (W, W), (A, W)]:
        layers.append((flat[at:at + o * i].reshape(o, i), flat[at + o * i:at + o * i + o]))
        at += o * i + o
    assert at == flat.size
    x = np.asarray(obs, np.float64)
    for w, b in layers[:D + 1]:
        x = np.maximum(x @ w.T + b, 0.0)
    (wv1, bv1), (wv2, bv2), (wp1, bp1), (wp2, bp2) = layers[D + 1:]
    value = np.tanh(np.maximum(x @ wv1.T + bv1, 0.0) @ wv2.T + bv2)[:, 0]
    logits = np.maximum(x @ wp1.T + bp1, 0.0) @ wp2.T + bp2
    legal = np.asarray(legal, bool)
    top = np.where(legal.any(1, keepdims=True), np.where(legal, logits, -np.inf).max(1, keepdims=True), 0.0)
    e = np.where(legal, np.exp(np.where(legal, logits - top, 0.0)), 0.0)
    return e / np.maximum(e.sum(1, keepdims=True), 1e-300), value, logits


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("vpnet_plan") / "vpnet_plan_host_test")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover",
                           "-I", os.path.join(ROOT, "open_spiel_amd", "csrc"), os.path.join(ROOT, "tests", "native", "vpnet_plan_host_test.cpp"), "-o", exe])

    def run(shape, limit=LDS_LIMIT):
        out = subprocess.check_output([exe, *map(str, shape), str(limit)], text=True)
        return [line.split() for line in out.splitlines()]
    return run


@pytest.mark.parametrize("shape", [(27, 64, 0, 9), (126, 256, 1, 7), (729, 256, 2, 81), (1089, 512, 8, 121), (7, 1, 0, 1), (225, 40, 1, 26)])
def test_the_plan_fits_is_aligned_and_disjoint_and_keeps_the_bank_rule(plan, shape):
    O, W, D, A = shape
    lines = plan(shape)
    assert lines[0][0] == "ok", lines
    lds, R, MR, NC, KC, panel_stride, panel_rows, params = (int(x) for x in lines[0][1:9])
    W16, A16 = -(-W // 16) * 16, -(-A // 16) * 16
    assert lds <= LDS_LIMIT and R == 32 * MR and MR * NC <= 16 and 64 * NC >= W16 and KC in (4, 8, 16)
    assert panel_stride == KC and panel_rows == min(max(W16, A16), 64 * NC)
    assert panel_rows * KC <= 8 * 512 and R * KC <= 4 * 512                   # the threads' fetch registers hold a panel and a stage
    assert [int(l[1]) for l in lines if l[0] == "stride"] == [W16 + 4, A16 + 4]   # 4 mod 16: the bank argument of osg_vpnet_plan.h
    assert all(l[1:] == ["64", "64"] for l in lines if l[0] == "banks") and sum(l[0] == "banks" for l in lines) == KC // 4
    bufs = sorted((int(l[1]), int(l[2])) for l in lines if l[0] == "buf")
    assert all(start % 4 == 0 for start, _ in bufs)                            # 16 bytes
    assert all(a + n <= b for (a, n), (b, _) in zip(bufs, bufs[1:])) and (bufs[-1][0] + bufs[-1][1]) * 4 <= lds
    (x0, xn), (x1, _) = [(int(l[1]), int(l[2])) for l in lines if l[0] == "alias"]
    assert x0 == bufs[0][0] and x0 % 4 == 0 and x1 == x0 + xn and x1 + xn <= bufs[0][0] + bufs[0][1]   # both stages inside act
    sizes = [(W, O)] + [(W, W)] * D + [(W, W), (1, W), (W, W), (A, W)]
    assert [int(x) for x in lines[-1 - KC // 4][1:]] == list(np.cumsum([0] + [o * i + o for o, i in sizes])[:-1])
    assert params == sum(o * i + o for o, i in sizes)
    assert plan(shape) == lines                                                # a pure function of its arguments
    assert plan(shape, lds)[0] == lines[0]                                     # ... which takes the most rows that fit


def test_the_plan_refuses_with_a_reason_and_says_where_the_search_net_lands(plan):
    for shape, limit in (((126, 513, 1, 7), LDS_LIMIT), ((126, 256, 1, 385), LDS_LIMIT), ((2049, 256, 1, 7), LDS_LIMIT),
                         ((126, 256, 9, 7), LDS_LIMIT), ((126, 256, 1, 7), 16 * 1024), ((0, 256, 1, 7), LDS_LIMIT)):
        line = plan(shape, limit)[0]
        assert line[0] == "refused" and len(line) > 3, line
    assert plan((126, 256, 1, 7))[0][2:6] == ["128", "4", "4", "8"] and plan((729, 256, 1, 81))[0][2:3] == ["64"]
    assert plan((1089, 512, 1, 121))[0][2:3] == ["32"] and plan((126, 512, 1, 7))[0][2:3] == ["64"]


def test_vpnet_mlp_is_one_flat_parameter_and_matches_the_float64_restatement():
    from open_spiel_amd.alpha_zero import VPNetMLP
    torch.manual_seed(3)
    shape = O, W, D, A = 27, 20, 2, 9
    model = VPNetMLP(O, A, W, D, weight_decay=1e-3)
    params = list(model.parameters())
    assert len(params) == 1 and params[0] is model.flat and model.flat.dtype == torch.float32
    assert model.flat.numel() == (W * O + W) + D * (W * W + W) + 2 * (W * W + W) + (W + 1) + (A * W + A)
    assert all(w.data_ptr() >= model.flat.data_ptr() for w, _ in model.weights())   # views, not copies
    g = torch.Generator().manual_seed(5)
    obs = (torch.rand(33, O, generator=g) < 0.4).float()
    legal = torch.rand(33, A, generator=g) < 0.5
    legal[:, 0] |= ~legal.any(1)                    # (the reference's softmax has no row without a legal action)
    legal[1] = torch.arange(A) == 4
    policy, value = model(obs, legal)
    want_policy, want_value, logits = reference_forward(model.flat.detach().numpy(), shape, obs.numpy(), legal.numpy())
    assert np.abs(policy.detach().numpy() - want_policy).max() < 1e-6 and np.abs(value.detach().numpy() - want_value).max() < 1e-6
    assert (policy.detach().numpy()[~legal.numpy()] == 0.0).all()
    targets = torch.softmax(torch.rand(33, A, generator=g), 1) * legal
    targets = targets / targets.sum(1, keepdim=True)
    value_targets = torch.rand(33, generator=g) * 2 - 1
    policy_loss, value_loss, l2 = model.losses(obs, legal, targets, value_targets)
    masked = np.where(legal.numpy(), logits, -65536.0)
    log_softmax = masked - masked.max(1, keepdims=True) - np.log(np.exp(masked - masked.max(1, keepdims=True)).sum(1, keepdims=True))
    assert abs(policy_loss.item() - (-(targets.numpy().astype(np.float64) * log_softmax).sum(1)).mean()) < 1e-5
    assert abs(value_loss.item() - ((want_value - value_targets.numpy()) ** 2).mean()) < 1e-6
    want_l2 = sum(1e-3 * (w.detach().double() ** 2).sum().item() / 2 for w, _ in model.weights())
    assert abs(l2.item() - want_l2) < 1e-6 * max(1.0, want_l2)
    (policy_loss + value_loss + l2).backward()       # autograd reaches the flat parameter through the views
    assert model.flat.grad is not None and torch.isfinite(model.flat.grad).all() and (model.flat.grad != 0).any()
