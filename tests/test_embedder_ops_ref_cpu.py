"""tests/embedder_ops_ref.py is the right operation: its fp64 front end, layer norm, pooling head, GELU derivative and attention
agree with the fp32 oracle (oracle/wav2vec2_ref.py, itself pinned by the golden fixtures) to fp32 round-off, forward and
through torch.autograd, in both feature-extractor modes.  No GPU.

Bounds: the oracle is fp32 torch; its reductions run over at most 399 frames / 32 channels here, so its own error is a few
2^-24 relative per element -- 1e-5 of max|ref| forward.  The waveform gradient passes the normaliser's Jacobian, where two
sums over the clip cancel: 1e-4 of max|grad|."""
import pytest
import torch
import torch.nn.functional as F

import embedder_ops_ref as R
from addvisor_hip import synthetic as syn
from oracle import signal_ref, wav2vec2_ref

FWD, GRAD = 1e-5, 1e-4


def rel(a, ref):
    return ((a.double() - ref.double()).abs().max() / ref.double().abs().max()).item()


def one_layer(stable):
    """The tiny config cut down to feature-encoder layer 0, so that ``wav2vec2_ref.feature_encoder`` IS the front end."""
    cfg = syn.tiny_config(stable, conv_dim=(32,), conv_kernel=(10,), conv_stride=(5,))
    return cfg, syn.embedder_weights(cfg)


def ref_front(wave, L, sd, stable):
    p = "feature_extractor.conv_layers.0."
    w0 = sd[p + "conv.weight"][:, 0]
    if not stable:
        return R.frontend(wave, L, w0, 0, True, sd[p + "layer_norm.weight"], sd[p + "layer_norm.bias"])["out"]
    z = R.frontend(wave, L, w0, 1, True, bias=sd[p + "conv.bias"])["out"]
    return R.layernorm(z, sd[p + "layer_norm.weight"], sd[p + "layer_norm.bias"], 1e-5, act=True)


@pytest.fixture(autouse=True)
def _grad_on():
    """Other test modules switch autograd off for the whole process when they are imported."""
    with torch.enable_grad():
        yield


@pytest.mark.parametrize("stable", [False, True])
@pytest.mark.parametrize("n_in,L", [(2000, 2000), (1500, 2000), (2300, 2000)])
def test_frontend_matches_oracle(stable, n_in, L):
    cfg, sd = one_layer(stable)
    wave = syn.make_clips(3, n_in, seed=5) * torch.tensor([[1.0], [30.0], [0.01]]) + torch.tensor([[0.0], [0.0], [0.02]])
    w32 = wave.clone().requires_grad_(True)
    o32 = wav2vec2_ref.feature_encoder(signal_ref.zero_mean_unit_var_norm(signal_ref.pad_or_crop(w32, L)), sd, cfg).transpose(1, 2)
    w64 = wave.double().requires_grad_(True)
    o64 = ref_front(w64, L, sd, stable)
    assert o64.dtype == torch.float64 and tuple(o64.shape) == tuple(o32.shape) == (3, (L - 10) // 5 + 1, 32)
    e = rel(o32.detach(), o64.detach())
    r = torch.randn(o32.shape, generator=torch.Generator().manual_seed(1))
    g32, = torch.autograd.grad((o32 * r).sum(), w32)
    g64, = torch.autograd.grad((o64 * r.double()).sum(), w64)
    eg = max(rel(g32[b], g64[b]) for b in range(3))                       # per clip: the amplitudes differ by 3000x
    print(f"front end stable={stable} n_in={n_in}: forward rel {e:.2e}, waveform gradient rel {eg:.2e}")
    assert e <= FWD and eg <= GRAD
    if n_in > L:
        assert (g64[:, L:] == 0).all()


def test_frontend_saved_statistics():
    """stats / mr are what the definitions say, and normalize = 0 is the identity."""
    g = torch.Generator().manual_seed(2)
    wave, w0 = torch.randn(2, 333, generator=g) * 3 + 1, torch.randn(8, 10, generator=g)
    gamma, beta = torch.rand(8, generator=g) + 0.5, torch.randn(8, generator=g)
    f = R.frontend(wave, 330, w0, 0, True, gamma, beta)
    x = wave[:, :330].double()
    assert torch.allclose(f["stats"][:, 0], x.mean(1)) and torch.allclose(f["stats"][:, 1], 1 / (x.std(1) + 1e-7))
    assert torch.allclose(f["xhat"], signal_ref.zero_mean_unit_var_norm(x))
    z = f["z0"]
    assert tuple(z.shape) == (2, 65, 8)
    assert torch.allclose(f["mr"][..., 0], z.mean(1)) and torch.allclose(f["mr"][..., 1], (z.var(1, unbiased=False) + 1e-5) ** -0.5)
    assert torch.allclose(f["out"], F.gelu(F.group_norm(z.transpose(1, 2), 8, gamma.double(), beta.double(), 1e-5)).transpose(1, 2))
    raw = R.frontend(wave, 330, w0, 1, False)
    assert torch.equal(raw["xhat"], x) and torch.equal(raw["out"], raw["z0"]) and raw["mr"] is None
    assert torch.equal(raw["stats"], torch.tensor([[0.0, 1.0]] * 2, dtype=torch.float64))
    assert torch.equal(R.pad_or_crop(wave, 400)[:, 333:], torch.zeros(2, 67)) and torch.equal(R.pad_or_crop(wave, 400)[:, :333], wave)


@pytest.mark.parametrize("act", [False, True])
def test_layernorm_pool_gelu_attention_match_torch(act):
    g = torch.Generator().manual_seed(3)
    x, a = torch.randn(5, 64, generator=g) * 2 + 0.5, torch.randn(5, 64, generator=g)
    gamma, beta = torch.rand(64, generator=g) + 0.5, torch.randn(64, generator=g)
    y = F.layer_norm(x + a, (64,), gamma, beta, 1e-5)
    assert rel(F.gelu(y) if act else y, R.layernorm(x, gamma, beta, 1e-5, add=a, act=act)) <= FWD
    assert rel(F.layer_norm(x, (64,), gamma, beta, 1e-5), R.layernorm(x, gamma, beta, 1e-5)) <= FWD
    h, coef = torch.randn(3, 7, 64, generator=g), torch.randn(64, generator=g)
    lo, pr = wav2vec2_ref.logreg(h.mean(1), coef[None].numpy(), [0.25])
    logit, prob, pooled = R.pool_logreg(h, coef, 0.25)
    assert rel(lo[:, 0], logit) <= FWD and rel(pr[:, 0], prob) <= FWD and rel(h.mean(1), pooled) <= FWD
    z = torch.linspace(-6, 6, 241, dtype=torch.float64).requires_grad_(True)
    dz, = torch.autograd.grad(F.gelu(z).sum(), z)
    assert (R.gelu_grad(z.detach()) - dz).abs().max().item() <= 1e-12 and (R.gelu(z.detach()) - F.gelu(z.detach())).abs().max().item() <= 1e-12
    q, k, v = (torch.randn(2, 3, 17, 8, generator=g) for _ in range(3))
    ctx, p = R.attention(q, k, v)
    assert rel(F.scaled_dot_product_attention(q, k, v), ctx) <= FWD and torch.allclose(p.sum(-1), torch.ones(2, 3, 17, dtype=torch.float64))
