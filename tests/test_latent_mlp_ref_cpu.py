"""tests/latent_mlp_ref.py and the case list it keeps for tests/test_hip_latent_mlp.py, checked without a GPU:
  - the reference against a torch.nn.Sequential of the same modules in float64 with autograd, two training steps: 1e-10;
  - conditioning: a float32 restatement of the reference stays under HALF of every bar the GPU test holds the kernel to, at
    every value-checked case (a condition on the inputs: a case that fails it gets another seed or scale, never another bar);
  - the case list is fixed, and its launch plans reach the branches of csrc/latent_mlp.hip the GPU file is there for."""
import zlib

import numpy as np
import pytest
import torch

import latent_mlp_ref as R

G = R          # the case list, the launch plan and the bars stand beside the reference

TORCH_BAR = 1e-10


def _sequential(c, d):
    N, I, H, sig = c
    mods, width = [], I
    for l in range(3):
        mods += [torch.nn.Linear(width, H), torch.nn.BatchNorm1d(H, eps=G.EPS, momentum=G.MOMENTUM), torch.nn.LeakyReLU(0.2)]
        width = H
    mods.append(torch.nn.Linear(H, 1))
    if sig:
        mods.append(torch.nn.Sigmoid())
    net = torch.nn.Sequential(*mods).double().train()
    lins, bns = [net[0], net[3], net[6], net[9]], [net[1], net[4], net[7]]
    order = [m.weight for m in lins] + [m.bias for m in lins] + [b.weight for b in bns] + [b.bias for b in bns]
    with torch.no_grad():
        for p, v in zip(order, d.params):
            p.copy_(torch.from_numpy(v).double())
        for l, b in enumerate(bns):
            b.running_mean.copy_(torch.from_numpy(d.buffers[l]).double())
            b.running_var.copy_(torch.from_numpy(d.buffers[3 + l]).double())
    return net, order, bns


@pytest.mark.parametrize("c", [c for c in G.CASES + G.STAGE_ONLY if c[0] >= 2], ids=G.cid)
def test_reference_equals_torch_in_float64(c):
    """output, dz, every parameter gradient and the pre-norm activations of step 1; running mean and variance after 2 steps"""
    d = G.draw(c)
    net, order, bns = _sequential(c, d)
    pre = []
    hooks = [m.register_forward_hook(lambda m, i, o: pre.append(o.detach().numpy().copy())) for m in (net[0], net[3], net[6])]
    z = torch.from_numpy(d.z).double().requires_grad_(True)
    y = net(z)
    y.backward(torch.from_numpy(d.dout).double().reshape(-1, 1))
    for h in hooks:
        h.remove()
    r = R.step(d.z, d.params, d.buffers, d.dout, G.EPS, G.MOMENTUM, c[3])
    gmax = max(float(np.max(np.abs(g))) for g in r.grads)
    assert G.relerr(r.out, y.detach().numpy()[:, 0]) < TORCH_BAR
    assert G.relerr(r.dz, z.grad.numpy()) < TORCH_BAR
    for l in range(3):
        assert G.relerr(r.a[l], pre[l]) < TORCH_BAR
    for i, (g, p) in enumerate(zip(r.grads, order)):
        assert g.shape == tuple(p.shape)
        assert float(np.max(np.abs(g - p.grad.numpy()))) <= TORCH_BAR * gmax, i
    with torch.no_grad():
        net(z)
    r2 = R.step(d.z, d.params, list(r.run_mean) + list(r.run_var), d.dout, G.EPS, G.MOMENTUM, c[3])
    for l, b in enumerate(bns):
        assert G.relerr(r2.run_mean[l], b.running_mean.numpy()) < TORCH_BAR
        assert G.relerr(r2.run_var[l], b.running_var.numpy()) < TORCH_BAR
        assert int(b.num_batches_tracked) == 2
    assert G.relerr(r2.out, r.out) == 0                            # the running buffers do not enter a training-mode output


def test_stage_function_is_the_forward_of_step():
    c = G.CASES[2]
    d = G.draw(c)
    r = R.step(d.z, d.params, d.buffers, d.dout, G.EPS, G.MOMENTUM, c[3])
    P = [np.asarray(p, np.float64) for p in d.params]
    x = np.asarray(d.z, np.float64)
    for l in range(3):
        a, mean, rstd, x = R.stage(x, P[l], P[4 + l], P[8 + l], P[11 + l], G.EPS)
        assert np.array_equal(a, r.a[l]) and np.array_equal(mean, r.stats[l][0]) and np.array_equal(rstd, r.stats[l][1])
        assert np.allclose(a.var(axis=0), 1 / rstd ** 2 - G.EPS, rtol=1e-12, atol=0)      # the biased variance
    assert np.array_equal(R.head(x, P[3], P[7], c[3]), r.out)


def test_a_batch_of_one_follows_the_library_convention():
    d = G.draw((1, 16, 64, False))
    r = R.step(d.z, d.params, d.buffers, d.dout, G.EPS, G.MOMENTUM, False)
    assert np.allclose(r.stats[:, 1], G.EPS ** -0.5, rtol=1e-14) and np.array_equal(r.stats[:, 0], r.a[:, 0])
    assert np.allclose(r.run_var, (1 - G.MOMENTUM) * np.stack(d.buffers[3:]).astype(np.float64), rtol=1e-14)
    assert np.all(r.dz == 0)


def _value_checked():
    """(id, case, key of the draw) of everything the GPU file compares end to end"""
    out = [(G.cid(c), c, None) for c in G.CASES]
    out += [(G.module_key(*m), m + (False,), G.module_key(*m)) for m in G.MODULE_CASES]
    return out


@pytest.mark.parametrize("name,c,key", _value_checked(), ids=[v[0] for v in _value_checked()])
def test_float32_restatement_stays_under_half_of_every_gpu_bar(name, c, key):
    """conditioning guard: the inputs, not the kernel, decide whether an fp32 implementation can meet the bars"""
    d = G.draw(c, key)
    r = R.step(d.z, d.params, d.buffers, d.dout, G.EPS, G.MOMENTUM, c[3])
    k = R.step(d.z, d.params, d.buffers, d.dout, G.EPS, G.MOMENTUM, c[3], dtype=np.float32)
    assert k.out.dtype == np.float32 and all(g.dtype == np.float32 for g in k.grads) and k.dz.dtype == np.float32
    e = G.value_errors(k, r)
    for q, v in e.items():
        assert v < 0.5 * G.BARS[q], (name, q, v)
    if key is not None:                                            # the module test runs a second step from the moved buffers
        bufs = list(r.run_mean) + list(r.run_var)
        r2 = R.step(d.z, d.params, bufs, d.dout, G.EPS, G.MOMENTUM, c[3])
        k2 = R.step(d.z, d.params, [np.float32(b) for b in list(k.run_mean) + list(k.run_var)], d.dout, G.EPS, G.MOMENTUM, c[3],
                    dtype=np.float32)
        for q, v in G.value_errors(k2, r2).items():
            assert v < 0.5 * G.BARS[q], (name, "step 2", q, v)


def test_case_list_is_fixed_and_plans_cover_the_branches():
    ids = [G.cid(c) for c in G.CASES + G.STAGE_ONLY]
    assert len(set(ids)) == len(ids) == 31
    assert zlib.crc32("\n".join(ids).encode()) == IDS_CRC, zlib.crc32("\n".join(ids).encode())
    a, b = G.draw(G.CASES[5]), G.draw(G.CASES[5])
    assert all(np.array_equal(x, y) for x, y in zip([a.z, a.dout] + a.params + a.buffers, [b.z, b.dout] + b.params + b.buffers))
    assert zlib.crc32(a.z.tobytes()) == DRAW_CRC, zlib.crc32(a.z.tobytes())
    assert all(c[0] >= 4 for c in G.CASES) and sorted(set(c[0] for c in G.STAGE_ONLY)) == [1, 2, 3]
    assert all(G.supported(*c[:3]) and c[0] * c[2] <= 4096 for c in G.CASES + G.STAGE_ONLY)
    assert all(G.supported(*m) for m in G.MODULE_CASES) and all(c in G.CASES for c in G.CONTRACT)
    assert sorted(set(c[2] for c in G.CONTRACT)) == [16, 32, 64, 128] and any(c[3] for c in G.CONTRACT) and not all(c[3] for c in G.CONTRACT)
    nsig = sum(c[3] for c in G.CASES)
    assert len(G.CASES) // 4 <= nsig <= len(G.CASES) // 2
    assert G.EXTRA == (0, 3)                                        # ldz = I and ldz > I, every case
    plans = [(c,) + (G.plan(*c[:3]),) for c in G.CASES]
    # every J instance with all its 256 J slots live, and with part of the tile masked; every rounded-up J
    for J in G.J_INSTANCES:
        assert any(p["J"] == J and p["full"] for _, p in plans), J
        assert any(p["J"] == J and not p["full"] for _, p in plans), J
    assert set((p["need"], p["J"]) for _, p in plans if p["need"] != p["J"]) >= {(3, 4), (5, 8), (9, 16), (10, 16)}
    assert sorted(set(c[2] for c, _ in plans)) == [16, 32, 64, 128]
    assert sorted(set(p["nstep"] for _, p in plans)) == [2, 4, 8, 16]
    # the weight-gradient block's kb loop: one pass, and four at H = 128 (also with K = I = H in the first layer)
    assert set(p["kb"] for _, p in plans) == {1, 4} and any(p["kb_first"] == 4 for _, p in plans)
    assert all((p["kb"] == 4) == (c[2] == 128) for c, p in plans)
    # more than 64 KB of dynamic LDS, in each direction; the forward only at H = 128
    assert any(p["lds_fwd"] > G.LDS_DEFAULT for _, p in plans) and any(p["lds_fwd"] <= G.LDS_DEFAULT for _, p in plans)
    assert any(p["lds_bwd"] > G.LDS_DEFAULT and p["lds_fwd"] <= G.LDS_DEFAULT for _, p in plans)
    assert max(p["lds_bwd"] for _, p in plans) == G.lds_bytes(32, 128)[1] <= G.LDS_BUDGET
    assert not G.supported(33, 16, 128) or 33 * 128 > 4096
    # threads without an element; the head loop's 16-lane groups leaving at different trips at H = 16
    assert any(p["idle"] > 0 for _, p in plans) and any(p["idle"] == 192 for _, p in plans)
    assert any(c[2] == 16 and p["head_uneven"] for c, p in plans)
    # the first layer's width: 1, below nstep, H; the head's fold with one trip (H = 16)
    assert any(c[1] == 1 for c, _ in plans) and any(1 < c[1] < p["nstep"] for c, p in plans)
    for H in (16, 32, 64, 128):
        assert any(c[1] == c[2] == H for c, _ in plans), H
    # H = 256 passes the arithmetic half of the predicate and never the LDS half
    assert all(not G.supported(N, 16, 256) for N in range(1, 17)) and 256 * 257 * 4 > G.LDS_BUDGET


IDS_CRC = 1596570246      # zlib.crc32 of the ids of CASES + STAGE_ONLY, one per line
DRAW_CRC = 2316675995     # ... of the bytes of the z drawn for CASES[5]
