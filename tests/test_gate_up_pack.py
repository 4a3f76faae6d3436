"""CPU: pack.merge_gate_up / pack.split_gate_up (the merged gate / up layer of include/mixq.h mixq_gemm_mixed_gate_up_typed) -- the row
formula against an explicit loop, the round trip bit for bit in both types and both containers, every ValueError -- and the restatement
helper (tests/gate_up_restate.py) on a case small enough to work out by hand."""
import numpy as np
import pytest

import gate_up_restate as G

torch = pytest.importorskip("torch")
from mixq_tensorrt_llm_amd import pack  # noqa: E402

S = G.S


def layer(N, K, O, bf, seed, as_torch=False):
    rng = np.random.default_rng(seed)
    d = dict(weight=rng.integers(-127, 128, (N, K)).astype(np.int8),
             weights_scaling_factor=rng.uniform(0.001, 0.01, N).astype(np.float16),
             fp_weight=S.rn(rng.standard_normal((N, O)).astype(np.float32), True) if bf else rng.standard_normal((N, O)).astype(np.float16),
             fp_ind=np.arange(O, dtype=np.int32) * 3)
    if as_torch:
        d = {k: torch.from_numpy(v.view(np.int16) if v.dtype == np.uint16 else v) for k, v in d.items()}
        if bf:
            d["fp_weight"] = d["fp_weight"].view(torch.bfloat16)
    return d


def raw(a):
    if isinstance(a, torch.Tensor):
        a = (a.view(torch.int16) if a.dtype in (torch.float16, torch.bfloat16) else a).numpy()
    return np.ascontiguousarray(a).view(np.uint8)


def test_the_row_formula_against_an_explicit_loop():
    for N in (16, 32, 48, 1040):
        r = pack.gate_up_rows(N)
        assert r.tolist() == [16 * (n // 8) + n % 8 for n in range(N)]
        both = sorted(r.tolist() + (r + 8).tolist())
        assert both == list(range(2 * N))                      # a permutation of the 2N merged rows
    assert pack.gate_up_rows(16).tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 16, 17, 18, 19, 20, 21, 22, 23]


@pytest.mark.parametrize("as_torch", [False, True], ids=["numpy", "torch"])
@pytest.mark.parametrize("bf", [False, True], ids=["fp16", "bf16"])
def test_merge_matches_the_loop_and_split_inverts_it(bf, as_torch):
    N, K, O = 48, 64, 8
    g, u = layer(N, K, O, bf, 1, as_torch), layer(N, K, O, bf, 2, as_torch)
    m = pack.merge_gate_up(g, u)
    assert sorted(m) == ["fp_ind", "fp_weight", "weight", "weights_scaling_factor"]
    for key in ("weight", "weights_scaling_factor", "fp_weight"):
        assert type(m[key]) is type(g[key]) and m[key].dtype == g[key].dtype and m[key].shape[0] == 2 * N
        want = G.merge_rows(raw(g[key]).reshape(N, -1), raw(u[key]).reshape(N, -1))
        assert np.array_equal(raw(m[key]).reshape(2 * N, -1), want), key
    assert np.array_equal(raw(m["fp_ind"]), raw(g["fp_ind"]))
    g2, u2 = pack.split_gate_up(m)
    for key in ("weight", "weights_scaling_factor", "fp_weight", "fp_ind"):
        assert np.array_equal(raw(g2[key]), raw(g[key])) and np.array_equal(raw(u2[key]), raw(u[key])), key
        assert g2[key].dtype == g[key].dtype and tuple(g2[key].shape) == tuple(g[key].shape)


def test_every_value_error():
    N, K, O = 32, 64, 8
    g = layer(N, K, O, False, 1)

    def other(**kw):
        u = layer(kw.pop("N", N), kw.pop("K", K), kw.pop("O", O), kw.pop("bf", False), 2)
        u.update(kw)
        return u

    with pytest.raises(ValueError, match="32 x 64"):
        pack.merge_gate_up(g, other(K=128))
    with pytest.raises(ValueError, match="32 x 64"):
        pack.merge_gate_up(g, other(N=48))
    with pytest.raises(ValueError, match="fp_weight"):
        pack.merge_gate_up(g, other(bf=True))                                      # fp16 gate, bf16 up
    with pytest.raises(ValueError, match="weights_scaling_factor"):
        pack.merge_gate_up(g, other(weights_scaling_factor=g["weights_scaling_factor"].astype(np.float32)))
    with pytest.raises(ValueError, match="fp_weight"):
        pack.merge_gate_up(g, {**other(), "fp_weight": torch.from_numpy(g["fp_weight"])})  # one container per key
    with pytest.raises(ValueError, match="fp_ind"):
        pack.merge_gate_up(g, other(fp_ind=g["fp_ind"] + 1))
    with pytest.raises(ValueError, match="fp_ind"):
        pack.merge_gate_up(g, other(O=16))
    with pytest.raises(ValueError, match="multiple of 16"):
        pack.merge_gate_up(layer(24, K, O, False, 1), layer(24, K, O, False, 2))
    for a, b in ((dict(g, bias=np.zeros(N, np.float16)), other()), (g, other(bias=np.zeros(N, np.float16)))):
        with pytest.raises(ValueError, match="bias"):
            pack.merge_gate_up(a, b)
    assert pack.merge_gate_up(dict(g, bias=None), other())["weight"].shape == (2 * N, K)  # (a None bias is no bias)
    m = pack.merge_gate_up(g, other())
    with pytest.raises(ValueError, match="blocks"):
        pack.split_gate_up({k: (v[:48] if k != "fp_ind" else v) for k, v in m.items()})
    with pytest.raises(ValueError, match="rows"):
        pack.split_gate_up(dict(m, fp_weight=m["fp_weight"][:32]))


@pytest.mark.parametrize("bf", [False, True], ids=["fp16", "bf16"])
def test_restatement_on_a_case_worked_out_by_hand(bf):
    """One row, N = 16: acc = 8 on every merged row, sW sA = 0.125 on gate rows and 0.25 on up rows, P = 6 on gate row 3 only."""
    N = 16
    q = np.array([[3, -2, 1, 0] * 4], np.int8)
    W2 = np.tile(np.array([1, 1, 1, 1] * 4, np.int8), (2 * N, 1))
    sA = S.rn(np.array([0.5], np.float32), bf)
    r = G.merged_rows(N)
    sW2 = np.empty(2 * N, np.float16)
    sW2[r], sW2[r + 8] = 0.25, 0.5
    fpA = S.rn(np.array([[3.0, 5.0]], np.float32), bf)
    fpW2 = np.zeros((2 * N, 2), np.float32)
    fpW2[G.merged_row(3)] = [2.0, 0.0]
    fpW2 = S.rn(fpW2, bf)
    got = G.gate_up_bits(q, sA, fpA, W2, sW2, fpW2, bf)
    vg = np.full(N, 1.0, np.float32)
    vg[3] = 7.0
    want = S.mul_bits(S.silu_bits(vg, bf), S.rn(np.full(N, 2.0, np.float32), bf), bf)
    assert got.shape == (1, N) and np.array_equal(got[0], want)
    assert np.array_equal(G.gate_up_bits(q, sA, None, W2, sW2, None, bf)[0], S.mul_bits(S.silu_bits(np.full(N, 1.0, np.float32), bf), S.rn(np.full(N, 2.0, np.float32), bf), bf))
    # an expf handed in replaces numpy's
    assert np.array_equal(G.gate_up_bits(q, sA, fpA, W2, sW2, fpW2, bf, expf=lambda x: np.exp(x, dtype=np.float32)), got)
    zero = G.gate_up_bits(q, sA, fpA, W2, sW2, fpW2, bf, expf=lambda x: np.full_like(x, np.inf))
    assert (zero[0] & 0x7FFF == 0).all()
