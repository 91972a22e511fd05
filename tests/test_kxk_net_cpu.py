"""CPU checks for the networks with 5 x 5 and 7 x 7 convs (asr_net_config.kernel_size / conv1_kernel_size):

  1. the fp64 restatement tests/kxk_net_oracle.py is pinned: equal to O.net_forward / O.net_backward at 3 x 3,
     and its gradients equal central finite differences of its own loss at k1 != kb;
  2. a CPU emulation of bf16 storage keeps every gradient group of the bf16 GPU parity cases at or below 0.6 of
     the 2e-2 bar (so the GPU test does not sit on the bar because of its inputs);
  3. the C ABI's parameter counts, its refusals and the struct size;
  4. the lowering of models with such convs (analyze needs no GPU).
"""
import ctypes as ct
import os
import re

import numpy as np
import pytest

import kxk_net_oracle as KO
from helpers import bf16_round, grad_groups, rel_l2
from oracle import asr_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. the restatement ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,anti", [("general", True), ("general", False), ("regular", False)])
def test_restatement_equals_oracle_at_3x3(kind, anti):
    spec = KO.KNetSpec(C=6, L=2, h=0.5, gamma=-0.05 if anti else 0.0, H=7, W=9, kind=kind, antisymmetric=anti)
    ospec = O.NetSpec(C=6, L=2, h=0.5, gamma=spec.gamma, H=7, W=9, kind=kind, antisymmetric=anti)
    rng = np.random.default_rng(3)
    params = KO.init_params(spec, rng)
    assert [p.shape for p in params] == [tuple(s) for s in ospec.param_shapes()]
    imgs, onehot = KO.make_batch(spec, 3, rng)
    probs, cache = KO.net_forward(spec, params, imgs)
    oprobs, ocache = O.net_forward(ospec, params, imgs)
    assert np.abs(probs - oprobs).max() <= 1e-12
    assert abs(KO.net_loss(probs, onehot) - O.net_loss(oprobs, onehot)) <= 1e-12
    for a, b in zip(KO.net_backward(spec, params, cache, onehot), O.net_backward(ospec, params, ocache, onehot)):
        assert np.abs(a - b).max() <= 1e-12 * max(1.0, np.abs(b).max())


@pytest.mark.parametrize("k", [5, 7])
@pytest.mark.parametrize("anti", [True, False])
def test_literal_assembly_equals_map(k, anti):
    spec = KO.KNetSpec(C=4, kind="general", antisymmetric=anti, kb=k, gamma=-0.05)
    rng = np.random.default_rng(k)
    theta = [rng.standard_normal(s) for s in spec.theta_shapes()]
    src, sign = spec.map()
    assert np.array_equal(O.assemble_general_literal(theta, 4, k, -0.05, anti),
                          O.assemble_from_map(O.flatten(theta), 4, src, sign, -0.05, k))


@pytest.mark.parametrize("k1,kb,kind,anti", [(5, 7, "general", True), (7, 5, "general", False), (7, 5, "regular", False)])
def test_restatement_gradients_match_finite_differences(k1, kb, kind, anti):
    spec = KO.KNetSpec(C=4, L=2, h=0.25, gamma=-0.05 if anti else 0.0, H=6, W=5, kind=kind, antisymmetric=anti,
                       k1=k1, kb=kb)
    rng = np.random.default_rng(11)
    params = KO.init_params(spec, rng)
    imgs, onehot = KO.make_batch(spec, 2, rng)
    probs, cache = KO.net_forward(spec, params, imgs)
    grads = KO.net_backward(spec, params, cache, onehot)
    assert [g.shape for g in grads] == [p.shape for p in params]

    def loss_at(ps):
        return KO.net_loss(KO.net_forward(spec, ps, imgs)[0], onehot)
    eps = 1e-5
    for t, (p, g) in enumerate(zip(params, grads)):
        scale = max(np.abs(g).max(), 1e-30)
        for idx in rng.choice(p.size, size=min(p.size, 4), replace=False):
            hi = [q.copy() for q in params]
            lo = [q.copy() for q in params]
            hi[t].flat[idx] += eps
            lo[t].flat[idx] -= eps
            fd = (loss_at(hi) - loss_at(lo)) / (2 * eps)
            assert abs(fd - g.flat[idx]) <= 1e-6 * scale, (t, idx, fd, g.flat[idx])


# ---- 2. the bf16 cases do not sit on the bar ------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(KO.BF16_CASES)))
def test_bf16_cases_emulated_below_six_tenths_of_the_bar(case):
    spec, params, imgs, onehot = KO.bf16_case(case)
    probs, cache = KO.net_forward(spec, params, imgs)
    want = KO.net_backward(spec, params, cache, onehot)

    def rnd(a):
        return bf16_round(a).astype(np.float64)
    eprobs, ecache = KO.net_forward(spec, params, imgs, rnd=rnd, rnd_w=rnd)
    got = KO.net_backward(spec, params, ecache, onehot, rnd=rnd)
    worst = max((rel_l2(a, b), name) for (name, a), (_, b) in zip(grad_groups(spec, got), grad_groups(spec, want)))
    print(f"case {case} {KO.BF16_CASES[case]}: worst group {worst[1]} rel-L2 {worst[0]:.2e}")
    assert worst[0] <= 1.2e-2, worst
    assert np.abs(eprobs - probs).max() < 1e-2


# ---- 3. the C ABI -----------------------------------------------------------------------------------------------------
def _cfg(**kw):
    from differential_equations_resnet_amd import _lib
    d = dict(N=2, H=8, W=32, Cin=3, C=16, L=2, num_classes=10, h=0.5, gamma=0.0, subtract_mean=0.0,
             divide_by_stddev=1.0, use_norm=0, dtype=_lib.ASR_F32, input_u8=1, param_kind=_lib.ASR_PARAM_GENERAL,
             antisymmetric=1, integrator=0, variant=0, kernel_size=0, conv1_kernel_size=0)
    d.update(kw)
    return _lib.NetConfig(**d)


@pytest.fixture(scope="module")
def lib():
    from differential_equations_resnet_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("k1,kb,kind,anti", [(5, 5, "general", True), (7, 7, "general", False), (5, 7, "regular", False),
                                             (7, 3, "3by3", True), (3, 5, "general", True)])
def test_param_count_equals_counted_shapes(lib, k1, kb, kind, anti):
    spec = KO.KNetSpec(C=16, L=2, kind=kind, antisymmetric=anti, k1=k1, kb=kb)
    c = _cfg(param_kind=spec.param_kind(), antisymmetric=int(anti), kernel_size=kb, conv1_kernel_size=k1)
    assert lib.asr_net_param_count(ct.byref(c)) == spec.n_params()
    assert lib.asr_net_workspace_bytes(ct.byref(c)) > 0
    inf = _cfg(param_kind=spec.param_kind(), antisymmetric=int(anti), kernel_size=kb, conv1_kernel_size=k1, variant=32)
    assert 0 < lib.asr_net_workspace_bytes(ct.byref(inf)) < lib.asr_net_workspace_bytes(ct.byref(c))


@pytest.mark.parametrize("dtype", [0, 1])
def test_sizes_zero_and_three_are_the_same_network(lib, dtype):
    base = dict(dtype=dtype, param_kind=0, H=32)
    a, b = _cfg(**base), _cfg(kernel_size=3, conv1_kernel_size=3, **base)
    assert lib.asr_net_param_count(ct.byref(a)) == lib.asr_net_param_count(ct.byref(b)) > 0
    assert lib.asr_net_workspace_bytes(ct.byref(a)) == lib.asr_net_workspace_bytes(ct.byref(b)) > 0


@pytest.mark.parametrize("kw,code", [
    (dict(kernel_size=4), -1), (dict(conv1_kernel_size=4), -1), (dict(kernel_size=9), -2),
    (dict(conv1_kernel_size=9), -2), (dict(kernel_size=5, param_kind=0), -1),
    (dict(kernel_size=5, dtype=1, W=24), -2), (dict(kernel_size=7, dtype=1, C=12), -2),
    (dict(kernel_size=5, integrator=1), -2)])
def test_refusals_name_the_accepted_set(lib, kw, code):
    from differential_equations_resnet_amd import _lib
    c = _cfg(**kw)
    assert lib.asr_net_param_count(ct.byref(c)) == -1
    assert lib.asr_net_workspace_bytes(ct.byref(c)) == 0
    assert lib.asr_net_prepare(ct.byref(c), None, 0) == code  # (the config check comes before the workspace's)
    msg = _lib.last_error()
    assert "{0 (= 3), 3, 5, 7}" in msg and "W in {8, 16, 32}" in msg, msg


def test_rk2_with_a_large_conv1_is_accepted(lib):
    c = _cfg(conv1_kernel_size=7, integrator=1, param_kind=0)
    assert lib.asr_net_param_count(ct.byref(c)) == KO.KNetSpec(C=16, L=2, kind="3by3", k1=7).n_params()


def test_struct_size_matches_header():
    from differential_equations_resnet_amd import _lib
    text = open(os.path.join(ROOT, "include", "asr.h")).read()
    body = re.search(r"typedef struct asr_net_config \{(.*?)\} asr_net_config;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip() for decl in body.split(";") if decl.strip()
             for n in re.sub(r"^\s*(int|float)\s", "", decl.strip()).split(",")]
    assert names == [f[0] for f in _lib.NetConfig._fields_]
    assert names[-2:] == ["kernel_size", "conv1_kernel_size"]
    assert ct.sizeof(_lib.NetConfig) == 4 * len(names)


# ---- 4. lowering -----------------------------------------------------------------------------------------------------
_hand_built = KO.hand_built_model


def _count(lib, plan, N=2, dtype=0):
    c = _cfg(N=N, H=plan.H, W=plan.W, Cin=plan.Cin, C=plan.C, L=plan.L, num_classes=plan.num_classes,
             param_kind=plan.param_kind, antisymmetric=int(plan.antisymmetric), dtype=dtype,
             kernel_size=plan.kernel_size, conv1_kernel_size=plan.conv1_kernel_size)
    return lib.asr_net_param_count(ct.byref(c))


def test_lowering_of_the_builder_and_of_hand_built_models(lib):
    from differential_equations_resnet_amd import _lib
    from differential_equations_resnet_amd.lowering import analyze
    from differential_equations_resnet_amd.models.tfkeras_resnets import build_single_block_resnet
    one = dict(num_stages=2, blocks_per_stage=[2], filters_per_block=[16], strides=[(1, 1)], num_classes=10, h=0.25)
    m = build_single_block_resnet((32, 32, 3), kernel_type="antisymmetric", kernel_size=5, **one)
    p = analyze(m)
    assert (p.conv1_kernel_size, p.kernel_size, p.param_kind) == (5, 3, _lib.ASR_PARAM_3BY3)
    assert sum(v.value.size for v in p.weight_vars()) == _count(lib, p)
    m = build_single_block_resnet((32, 32, 3), kernel_type="regular", kernel_size=7, **one)
    p = analyze(m)
    assert (p.conv1_kernel_size, p.kernel_size, p.param_kind) == (7, 7, _lib.ASR_PARAM_REGULAR)
    assert sum(v.value.size for v in p.weight_vars()) == _count(lib, p) == _count(lib, p, dtype=1)
    p = analyze(_hand_built([3, 5, 5]))
    assert (p.conv1_kernel_size, p.kernel_size, p.param_kind, p.L) == (3, 5, _lib.ASR_PARAM_GENERAL, 2)
    assert sum(v.value.size for v in p.weight_vars()) == _count(lib, p)


def test_lowering_refusals_name_the_layer():
    from differential_equations_resnet_amd import _lib, graph as G
    from differential_equations_resnet_amd.lowering import analyze
    from differential_equations_resnet_amd.models.tfkeras_resnets import build_single_block_resnet
    with pytest.raises(_lib.AsrUnsupported, match="blk1.*kernel size"):
        analyze(_hand_built([3, 5, 7]))
    with pytest.raises(_lib.AsrUnsupported, match="blk0.*kernel size"):
        analyze(_hand_built([3, 9]))
    inp = G.Input((16, 16, 3))
    x = G.Activation("relu")(G.Conv2D(filters=8, kernel_size=(5, 3), padding="same", name="conv1")(inp))
    y = G.Activation("relu")(G.Conv2D(filters=8, kernel_size=3, padding="same", name="b0")(x))
    x = G.GlobalAveragePooling2D()(G.add([y, x]))
    with pytest.raises(_lib.AsrUnsupported, match="conv1"):
        analyze(G.Model(inp, G.Dense(10, activation="softmax", name="fc")(x)))
    # kernel_size=9: the walk from the output meets the regular block conv first, conv1 with the 3by3 blocks
    for kernel_type, layer in (("regular", "res2_0_branch2"), ("antisymmetric", "conv1")):
        with pytest.raises(_lib.AsrUnsupported, match=layer + ".*kernel size"):
            analyze(build_single_block_resnet((32, 32, 3), kernel_type=kernel_type, kernel_size=9, num_stages=2,
                                              blocks_per_stage=[1], filters_per_block=[16], strides=[(1, 1)],
                                              num_classes=10))
    with pytest.raises(_lib.AsrUnsupported, match=r"3x3"):
        analyze(build_single_block_resnet((32, 32, 3), kernel_type="regular", kernel_size=5, num_stages=4,
                                          blocks_per_stage=[1, 1, 1], filters_per_block=[16, 32, 64],
                                          strides=[(1, 1), (2, 2), (2, 2)], num_classes=10))
