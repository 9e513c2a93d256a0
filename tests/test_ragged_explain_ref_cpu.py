"""CPU-only: the claims of the ragged explanation tests' length table (tests/ragged_explain_ref.py), the host-side refusals of the
ragged pipeline, and that the per-clip-alone reference tells the padded-batch mistake apart."""
import inspect

import pytest
import torch

import ragged_explain_ref as R
from addvisor_hip import ops, synthetic as syn
from addvisor_hip.embedder import HipEmbedder
from addvisor_hip.pipeline import ExplainPipeline
from addvisor_hip.unet import HipUNet

torch.set_grad_enabled(False)


def bare_pipeline():
    """The host checks need no device."""
    emb = HipEmbedder.__new__(HipEmbedder)
    emb.cfg = R.models()[0]
    pipe = ExplainPipeline.__new__(ExplainPipeline)
    pipe.embedder, pipe.hop, pipe.win, pipe.L, pipe.vocoder = emb, R.HOP, R.WIN, R.L, None
    return pipe


def test_table_claims():
    T, Wd = R.frame_counts(R.L)
    assert (T, Wd) == (25, 24) and R.H == 512
    assert [(n,) + R.frame_counts(n) for n in R.LENGTHS] == [row[:3] for row in R.TABLE]
    assert R.LENGTHS == (8000, 7999, 7728, 7727, 6440, 5151, 2576, 1288, 966)
    assert 7728 == 24 * R.HOP and R.frame_counts(7727)[0] == 24                     # the boundary between 24 and 25 frames
    assert {w for _, _, w, _ in R.TABLE} == {24, 20, 16, 8, 4}                      # every width class of a 24-column buffer but 12
    assert R.frame_counts(R.TOO_SHORT) == (3, 0)
    assert R.clips().shape == (9, R.L)


def test_every_clip_alone_is_finite_and_has_its_shapes():
    ref = R.table_reference()
    for b, (n, Tb, Wb, _) in enumerate(R.TABLE):
        assert torch.isfinite(torch.view_as_real(ref["spec"][b])).all() and torch.isfinite(ref["mask"][b]).all()
        assert ref["mag"][b, :, :Tb].abs().amax(0).min() > 0                         # every own frame is live
        assert (ref["mag"][b, :, Tb:] == 0).all() and (ref["mask"][b, :, Wb:] == 0).all()
        assert (ref["wave_in"][b, n:] == 0).all() and (ref["wave_out"][b, n:] == 0).all()
        assert ref["mask"][b, :, :Wb].min() > 0                                      # a sigmoid: the zeros above are the embedding's
    for k in R.PROBS:
        assert ref[k].shape == (9, 1) and torch.isfinite(ref[k]).all() and ((ref[k] > 0) & (ref[k] < 1)).all()
    # the full-length clip alone is the plain oracle
    from oracle import lmac_ref
    cfg, emb_sd, unet_sd, coef, icpt = R.models()
    plain = lmac_ref.explain(R.clips()[:1], emb_sd, cfg, coef, icpt, unet_sd, audio_length=R.L / 16000)
    assert torch.equal(plain["mask"][0], ref["mask"][0]) and torch.equal(plain["wave_in"][0], ref["wave_in"][0])
    assert torch.equal(plain["theta_out"][0], ref["theta_out"][0])


def test_too_short_fails():
    with pytest.raises(ValueError, match="no mask column"):
        R.explain_alone(R.clips()[0, :R.TOO_SHORT])
    pipe = bare_pipeline()
    assert pipe.min_length() == 966 == max(pipe.embedder.min_length(), 3 * R.HOP, 513)
    with pytest.raises(ValueError, match=r"clip 1 has 965 samples.*shortest supported length is 966"):
        pipe._check_lengths([8000, 965], 2)
    with pytest.raises(ValueError, match=r"clip 0 has 965"):
        pipe.frame_counts([965])
    assert pipe.frame_counts(list(R.LENGTHS)) == ([r[1] for r in R.TABLE], [r[2] for r in R.TABLE])
    assert pipe.frame_counts(torch.tensor(R.LENGTHS)) == ([r[1] for r in R.TABLE], [r[2] for r in R.TABLE])


def test_lengths_and_widths_validation_on_the_host():
    pipe = bare_pipeline()
    with pytest.raises(ValueError, match="2 entries for a batch of 3"):
        pipe._check_lengths([8000, 966], 3)
    with pytest.raises(ValueError, match="not an integer"):
        pipe._check_lengths([8000, 966.0], 2)
    with pytest.raises(ValueError, match="not an integer"):
        pipe._check_lengths([8000, True], 2)
    with pytest.raises(ValueError, match="integer tensor"):
        pipe._check_lengths(torch.tensor([8000.0, 966.0]), 2)
    with pytest.raises(ValueError, match="integer tensor"):
        pipe._check_lengths(7, 1)
    with pytest.raises(ValueError, match=r"lengths\[1\] = 8001 exceeds"):
        pipe._check_lengths([8000, 8001], 2)
    assert ops.min_clip_samples(322) == 966 and ops.min_clip_samples(256) == 768 and ops.min_clip_samples(100) == 513
    # explain refuses on the host, before anything touches a device: CPU tensors never get as far as a launch
    with pytest.raises(ValueError, match="CUDA fp32"):
        pipe.explain(torch.zeros(2, R.L), lengths=[8000, 966])
    cw = HipUNet._check_widths
    assert cw([24, 4, 12], 3, 24) == [24, 4, 12] and cw(torch.tensor([24, 8]), 2, 24) == [24, 8]
    import numpy as np
    assert cw(np.array([24, 8]), 2, 24) == [24, 8] and cw([np.int64(24), 8], 2, 24) == [24, 8]      # what check_clip_lengths accepts
    with pytest.raises(ValueError, match="integer tensor"):
        cw(np.array([24.0, 8.0]), 2, 24)
    for bad, msg in (([24, 4], "2 entries for a batch of 3"), ([24, 4, 0], "multiple of 4"), ([24, 4, 28], "multiple of 4"),
                     ([24, 4, 6], "multiple of 4"), ([24, 4, 8.0], "not an integer"), ([24, 4, True], "not an integer")):
        with pytest.raises(ValueError, match=msg):
            cw(bad, 3, 24)
    with pytest.raises(ValueError, match="integer tensor"):
        cw(torch.tensor([24.0]), 1, 24)
    for fn in (ops.stft_forward, ops.istft_masked_c64, ExplainPipeline.explain):
        assert inspect.signature(fn).parameters["lengths"].default is None
    assert inspect.signature(HipUNet.forward).parameters["widths"].default is None
    import LMAC_metrics
    assert inspect.signature(LMAC_metrics.explain_batch).parameters["lengths"].default is None
    assert "lengths" not in inspect.signature(ExplainPipeline.explain_graphed).parameters


def test_the_reference_tells_the_padded_batch_apart():
    ref, w = R.table_reference(), R.clips()
    for b, (n, Tb, Wb, _) in enumerate(R.TABLE):
        d = (R.padded_mask(w[b], n) - ref["mask"][b, :, :Wb]).abs().max().item()
        flips = ((R.padded_mask(w[b], n) > 0.5) != (ref["mask"][b, :, :Wb] > 0.5)).sum().item()
        print(f"{n} samples: padded mask vs alone, max |diff| {d:.3f} on the clip's {Wb} columns, {flips} entries of mask > 0.5 flip")
        if n <= 6440:
            assert d >= 0.5, (n, d)
        elif Tb == 25:
            assert d == 0.0, (n, d)
