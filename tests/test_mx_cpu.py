"""MX block-scaled storage on the host: ddstore_amd.mx against the float64
model (tests/mx_ref.py), bit for bit, and the host backend end to end."""
import numpy as np
import pytest
import torch

from ddstore_amd import mx
from tests import mx_ref
from tests.dist_utils import run_dist

DISPS = (1, 32, 33, 128, 1000)


def _same(got_f32, exp_f32):
    g, e = np.asarray(got_f32), np.asarray(exp_f32)
    return bool(np.all((g.view(np.uint32) == e.view(np.uint32)) | (np.isnan(g) & np.isnan(e))))


@pytest.mark.parametrize("disp", DISPS)
@pytest.mark.parametrize("elem", mx_ref.ELEMS)
def test_quantize_dequantize_match_model(elem, disp):
    x = mx_ref.inputs(45, disp)
    assert mx.row_bytes(disp, elem) == mx_ref.row_bytes(disp, elem)
    packed = mx.quantize(torch.from_numpy(x.copy()), elem).numpy()
    exp = mx_ref.quantize(x, elem)
    assert np.array_equal(packed, exp), np.argwhere(packed != exp)[:5]
    assert _same(mx.dequantize(torch.from_numpy(exp), disp, elem).numpy(),
                 mx_ref.decode(exp, disp, elem))


def _w_host(rank, world):
    from ddstore_amd import DDStore

    s = DDStore(device="cpu")
    x = mx_ref.inputs(40, 33)
    s.add_mx("v", torch.from_numpy(x[rank * 20:(rank + 1) * 20].copy()), elem="e2m1")
    q = s.query("v")
    assert (q["mx_elem"], q["mx_disp"], q["row_bytes"]) == ("e2m1", 33, 48)
    packed = mx_ref.quantize(x, "e2m1")
    assert np.array_equal(s.local_shard("v").numpy(), packed[rank * 20:(rank + 1) * 20])
    idx = np.array([39, 0, 21, 21, 3])
    dec = mx_ref.decode(packed, 33, "e2m1")[idx]
    assert _same(s.get_batch("v", idx).numpy(), dec)
    got = s.get_batch("v", idx, dtype=torch.bfloat16, affine=(0.5, 1.0))
    with np.errstate(invalid="ignore"):
        exp = (torch.from_numpy(dec) * 0.5 + 1.0).to(torch.bfloat16)
    assert torch.equal(got.view(torch.int16)[~exp.isnan()], exp.view(torch.int16)[~exp.isnan()])
    with pytest.raises(TypeError):
        s.get_batch("v", idx, dtype=torch.int32)
    with pytest.raises(TypeError):
        s.update("v", np.zeros((1, 48), np.uint8))
    s.free()


def test_host_backend_two_ranks():
    run_dist(_w_host, 2)
