"""The sinked ragged paged prefill against what honest arithmetic costs, as tests/test_accuracy_budget.py judges
every path: the same ``judge``, the same caps (derived there from CPU models over its kernel classes, not chosen
here), the same ``problem`` with ``sinks=True`` (``sink_logits``: randn + 2).

One ragged batch of three prompts read from their first token: chunks of 300 / 77 / 600 rows over 300 / 77 / 600 keys,
Hq 8, Hkv 2, D 128, causal, page 64.

The CPU part shows that an honest kernel cannot fail the caps on THIS shape: the honest "tiled" model with sinks (the
deferred-rescale arithmetic of fa_fwd_w4, the sink joining the final sum) stays at least ``SEPARATION`` (1.15 x)
below both caps on ``centered`` and ``sharp``, and its |bias| on ``offset`` 1.15 x below eps / 16.
"""
from __future__ import annotations

import functools

import pytest
import torch

from accuracy import EPS, NAMES
from test_accuracy_budget import DEV, DT_IDS, DTYPES, FAMS, PAGE, SEPARATION, caps, crc, dbg, judge, problem, to_pool  # noqa: F401

SQS = LENS = (300, 77, 600)
CAP = 640  # the key buffer: ten pages of 64
HQ, HKV, D = 8, 2, 128


@functools.lru_cache(maxsize=None)
def ragged_problem(fam, dtype):
    b = len(SQS)
    return problem(fam, dtype, b, HQ, HKV, max(SQS), CAP, D, crc("pvs", NAMES[dtype], fam), [0] * b, list(LENS), True,
                   qs=[0] * b, qe=list(SQS), sinks=True)


@pytest.mark.parametrize("fam", FAMS)
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_the_caps_stand_clear_of_the_honest_tiled_model_with_sinks(dtype, fam):
    p = ragged_problem(fam, dtype)
    assert p.sinks is not None and p.ref[0].numel() >= 16384
    rms, bias, emax = p.measure(p.run(dtype, variant="tiled")[0])
    h_rms, _, h_emax = p.measure(p.honest[0])
    print(f"MODEL pvarlen-sink {fam} {NAMES[dtype]} tiled: rms_ratio={rms / h_rms:.3f} emax_ratio={emax / h_emax:.3f} "
          f"bias={bias:.2e}")
    if fam == "offset":
        assert abs(bias) * SEPARATION <= EPS[dtype] / 16, bias
    else:
        rms_cap, emax_cap = caps(fam, dtype)[:2]
        assert rms / h_rms * SEPARATION <= rms_cap, (rms / h_rms, rms_cap)
        assert emax / h_emax * SEPARATION <= emax_cap, (emax / h_emax, emax_cap)


@pytest.mark.gpu
@pytest.mark.parametrize("fam", FAMS)
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_paged_varlen_sink(dbg, dtype, fam):  # noqa: F811
    """flash_attn_paged_varlen_func(..., sinks=): the ragged batch of the module docstring, causal."""
    from flash_attention_cute_amd import flash_attn_paged_varlen_func

    p = ragged_problem(fam, dtype)
    q = torch.cat([p.q[i, :, :s].transpose(0, 1) for i, s in enumerate(SQS)]).contiguous()
    cu = torch.tensor([0, 300, 377, 977], dtype=torch.int32)
    kc, vc, table, sl = to_pool(p, LENS, PAGE, 23)
    out = flash_attn_paged_varlen_func(q.to(DEV), kc.to(DEV), vc.to(DEV), cu.to(DEV), max(SQS), table.to(DEV), sl.to(DEV),
                                       causal=True, sinks=p.sinks.to(DEV))
    assert dbg.last_path() == "w4" and dbg.last_prefill_paged()
    out = out.cpu().double()
    unpack = torch.zeros(p.q.shape, dtype=torch.float64)
    for i, s in enumerate(SQS):
        unpack[i, :, :s] = out[int(cu[i]):int(cu[i + 1])].transpose(0, 1)
    judge("w4-paged-varlen-sink", p, unpack)
