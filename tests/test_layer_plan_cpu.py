"""CPU-only tests of the layer plan (modules.plan_sequence / plan_block): what the executors are told about every network
the project builds, parsed from the modules alone — no tensor, no GPU."""
import pytest
import torch.nn as nn

import dtgan_amd  # noqa: F401
from dtgan_amd import modules as M, networks as N, ops


def _split(plan):
    """-> (conv stages in front of the blocks, block stages, conv stages behind them)"""
    kinds = [isinstance(st, M.BlockStage) for st in plan]
    a = kinds.index(True)
    b = len(kinds) - kinds[::-1].index(True)
    assert all(kinds[a:b]) and not any(kinds[:a]) and not any(kinds[b:])
    return plan[:a], plan[a:b], plan[b:]


@pytest.mark.parametrize("stochastic", [False, True])
def test_generator_plan(stochastic):
    g = N.define_stochastic_G(16, 3, 3, 32, n_blocks=9) if stochastic else N.define_G(3, 3, 32, n_blocks=9)
    norm_cls = M.CondInstanceNorm if stochastic else M.InstanceNorm
    assert len(g.model) == 27
    stem, blocks, tail = _split(g.model.layer_plan())
    assert [(st.conv.kernel_size[0], st.conv.stride[0], st.reflect) for st in stem] == [(7, 1, 3), (3, 1, 0), (3, 2, 0)]
    for st in stem:
        assert type(st.conv) is M.Conv2d and type(st.norm) is norm_cls and st.act == ops.ACT_RELU and st.dropout is None
        assert st.norm in list(g.model)   # listed directly, not through a MergeModule
        assert not st.relu_feeds_conv     # the ReLU belongs to the norm
    assert [st.next_conv is not None for st in stem] == [True, True, False]
    assert stem[0].next_conv is stem[1].conv and stem[1].next_conv is stem[2].conv
    assert [st.next_block is not None for st in stem] == [False, False, True]
    assert stem[2].next_block is blocks[0].block
    assert len(blocks) == 9 and [st.last for st in blocks] == [False] * 8 + [True]
    assert all(type(st.block) is (M.CINResnetBlock if stochastic else M.ResnetBlock) for st in blocks)
    assert len(tail) == 3
    up, mid, head = tail
    assert type(up.conv) is M.ConvTranspose2d and type(up.norm) is norm_cls and up.act == ops.ACT_RELU
    assert type(mid.conv) is M.Conv2d and mid.conv.kernel_size[0] == 3 and type(mid.norm) is norm_cls and mid.act == ops.ACT_RELU
    assert up.next_conv is mid.conv and mid.next_conv is head.conv
    assert type(head.conv) is M.Conv2d and head.conv.kernel_size[0] == 7 and head.norm is None and head.act == ops.ACT_TANH
    assert head.next_conv is None and head.reflect == 0
    assert not any(st.next_block is not None or st.relu_feeds_conv or st.dropout is not None for st in tail)


@pytest.mark.parametrize("make", [lambda s: N.define_D_B(3, 64, "basic", "instance", use_sigmoid=s),
                                  lambda s: N.define_D_A(3, 32, "basic", "instance", use_sigmoid=s)])
@pytest.mark.parametrize("use_sigmoid", [False, True])
def test_discriminator_plan(make, use_sigmoid):
    d = make(use_sigmoid)
    assert len(d.model) == 12 + use_sigmoid
    plan = d.model.layer_plan()
    assert len(plan) == 5 and all(isinstance(st, M.ConvStage) and type(st.conv) is M.Conv2d for st in plan)
    assert [st.norm is None for st in plan] == [True, False, False, False, True]
    assert all(type(st.norm) is M.InstanceNorm for st in plan[1:4])
    assert [st.act for st in plan] == [ops.ACT_LRELU] * 4 + [ops.ACT_SIGMOID if use_sigmoid else ops.ACT_NONE]
    assert not any(st.relu_feeds_conv for st in plan)   # LeakyReLU is not linked
    assert [st.next_conv for st in plan] == [plan[1].conv, plan[2].conv, plan[3].conv, plan[4].conv, None]
    assert not any(st.reflect or st.dropout is not None or st.next_block is not None for st in plan)


def test_encoder_plan():
    e = N.define_E(16, 6, 32, "batch")
    assert len(e.conv_modules) == 14
    plan = e.conv_modules.layer_plan()
    assert len(plan) == 5 and all(isinstance(st, M.ConvStage) and type(st.conv) is M.Conv2d for st in plan)
    assert plan[0].norm is None and plan[0].act == ops.ACT_RELU
    assert [st.relu_feeds_conv for st in plan] == [True, False, False, False, False]   # conv + ReLU straight into a Conv2d
    assert all(type(st.norm) is M.BatchNorm2d and st.act == ops.ACT_RELU for st in plan[1:])
    assert [st.next_conv for st in plan] == [plan[1].conv, plan[2].conv, plan[3].conv, plan[4].conv, None]


@pytest.mark.parametrize("use_dropout", [False, True])
@pytest.mark.parametrize("padding_type", ["reflect", "zero"])
@pytest.mark.parametrize("cin", [False, True])
def test_block_plan(cin, padding_type, use_dropout):
    if cin:
        b = M.CINResnetBlock(32, 8, padding_type, M.CondInstanceNorm, use_dropout, True)
    else:
        b = M.ResnetBlock(32, padding_type, M.InstanceNorm2d, use_dropout, True)
    plan = b.layer_plan()
    assert len(plan) == 2 and all(isinstance(st, M.ConvStage) and type(st.conv) is M.Conv2d for st in plan)
    first, out = plan
    pad = 1 if padding_type == "reflect" else 0
    assert (first.reflect, out.reflect) == (pad, pad)
    assert first.conv.padding[0] == out.conv.padding[0] == 1 - pad
    mods = list(b.conv_block)
    assert first.dropout is (next(m for m in mods if isinstance(m, nn.Dropout)) if use_dropout else None)
    assert out.dropout is None
    if cin:
        merge = next(m for m in mods if isinstance(m, M.MergeModule))
        assert first.conv is merge.module1 and first.norm is merge.module2 and type(first.norm) is M.CondInstanceNorm
    else:
        assert first.norm is None
    assert first.act == ops.ACT_RELU
    # the link exists exactly for a conv + ReLU without a norm (a CINResnetBlock's ReLU belongs to its norm) whose output
    # reaches the second convolution without a Dropout in between
    assert first.relu_feeds_conv == (first.norm is None and not use_dropout)
    assert type(out.norm) is M.InstanceNorm and out.act == ops.ACT_NONE and not out.relu_feeds_conv
    assert first.next_conv is (out.conv if (pad == 0 and not use_dropout) else None)
    assert out.next_conv is None and first.next_block is None and out.next_block is None


def _conv(cin=16, cout=16, **kw):
    return M.Conv2d(cin, cout, kernel_size=3, padding=1, **kw)


def test_malformed_lists_are_refused_by_the_plan():
    with pytest.raises(NotImplementedError, match="unexpected layer Linear"):
        M.plan_sequence([_conv(), M.Linear(4, 4)])
    with pytest.raises(NotImplementedError, match="unexpected layer InstanceNorm"):
        M.plan_sequence([M.InstanceNorm(16), _conv()])
    with pytest.raises(NotImplementedError, match="reflection pad before ConvTranspose2d"):
        M.plan_sequence([nn.ReflectionPad2d(1), M.ConvTranspose2d(16, 16, kernel_size=3, stride=2, padding=1, output_padding=1)])
    with pytest.raises(NotImplementedError, match="LeakyReLU slope"):
        M.plan_sequence([_conv(), nn.LeakyReLU(0.1)])
    # inside a residual block
    with pytest.raises(NotImplementedError, match="residual fusion expects the block to end with its norm"):
        M.plan_block([_conv(), nn.ReLU(True), _conv(), M.InstanceNorm(16), nn.ReLU(True)])
    with pytest.raises(NotImplementedError, match="residual fusion expects the block to end with its norm"):
        M.plan_block([_conv(), nn.ReLU(True), _conv()])
    with pytest.raises(NotImplementedError, match="residual after CondInstanceNorm"):
        M.plan_block([_conv(), nn.ReLU(True), M.MergeModule(_conv(), M.CondInstanceNorm(16, 4))])
    with pytest.raises(NotImplementedError, match="residual block: expected"):
        M.plan_block([_conv(), M.InstanceNorm(16)])
    with pytest.raises(NotImplementedError, match="residual block: expected"):
        M.plan_block([M.ResnetBlock(16, "reflect", M.InstanceNorm2d, False, True), _conv(), M.InstanceNorm(16)])
    # ... and through the owner, before any tensor is involved
    b = M.ResnetBlock(16, "reflect", M.InstanceNorm2d, False, True)
    b.conv_block.add_module("7", nn.ReLU(True))
    with pytest.raises(NotImplementedError, match="end with its norm"):
        b.layer_plan()


def test_plan_is_cached_and_rebuilt_when_a_child_is_replaced():
    g = N.define_G(3, 3, 8)
    keys, rep, nmods = list(g.state_dict()), repr(g), len(list(g.modules()))
    plan = g.model.layer_plan()
    assert g.model.layer_plan() is plan and isinstance(plan, tuple)
    assert (list(g.state_dict()), repr(g), len(list(g.modules()))) == (keys, rep, nmods)   # a plain attribute
    new = M.Conv2d(8, 16, kernel_size=3, padding=1, stride=1, bias=True)
    g.model[4] = new
    plan2 = g.model.layer_plan()
    assert plan2 is not plan and plan2[1].conv is new and plan2[0].next_conv is new and plan[1].conv is not new
    assert g.model.layer_plan() is plan2
    blk = g.model[10]
    bplan = blk.layer_plan()
    assert blk.layer_plan() is bplan
    blk.conv_block[1] = M.Conv2d(32, 32, kernel_size=3, padding=0, bias=True)
    assert blk.layer_plan() is not bplan and blk.layer_plan()[0].conv is blk.conv_block[1]
    assert g.model.layer_plan() is plan2   # the block object itself is still the same child


def test_plan_holds_structure_only():
    """nothing that can change between two forwards of one module object: switches, train / eval mode"""
    g = N.define_G(3, 3, 8, use_dropout=True)
    gz = N.define_stochastic_G(4, 3, 3, 8, use_dropout=True)
    owners = [g.model, g.model[10], gz.model, gz.model[10], N.define_E(4, 6, 8, "batch").conv_modules]
    before = [o.layer_plan() for o in owners]
    switches = ["CONV_STATS_ENABLED", "DIRECT_GRAD", "LAZY_DRES", "NORM_SUMS", "RELU_LINK", "RELU_MASK", "S16_ENABLED",
                "NORM_SIGN_MASK", "COND_BANK", "LATENT_MLP"]
    saved = {k: getattr(ops, k) for k in switches}
    try:
        for k in switches:
            setattr(ops, k, not saved[k])
        g.eval(), gz.eval()
        for o, plan in zip(owners, before):
            assert o.layer_plan() is plan
            # a fresh parse under the flipped switches and in eval mode gives the same records, field by field: nothing
            # but the modules went into them
            fresh = o._planned()[1](o._planned()[0])
            assert fresh is not plan and fresh == plan
        assert before[1][0].dropout.training is False   # the module itself, read at run time
    finally:
        for k, v in saved.items():
            setattr(ops, k, v)
