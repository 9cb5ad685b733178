"""What the GPU tests of the pooler backward share (tests/test_gpu_pooler_bwd.py, tests/test_gpu_pooler_api.py)."""
import torch

from gpu_util import stream

POOL_W, POOL_B = "encoder.pooler.weight", "encoder.pooler.bias"
DEV = "cuda:0"


def launcher(eng, hid, d_pooled):
    """plb_launch_pooler_bwd on the bf16 image of position 0 of ``hid`` (at valid positions the fp32 hidden state IS the image
    of the bf16 rows the stash holds) and the engine's fp32 pooler parameters: (dW | db as one flat tensor, dh0)."""
    B, S, H = hid.shape
    hb = hid[:, 0].to(torch.bfloat16).contiguous()
    assert torch.equal(hb.float(), hid[:, 0])
    W, b = eng.view(POOL_W), eng.view(POOL_B)
    dpre, dh0 = torch.empty(B, H, device=DEV), torch.empty(B, H, device=DEV)
    dwb = torch.empty(H * H + H, device=DEV)
    dp = d_pooled.to(DEV).contiguous()
    assert eng.L.plb_launch_pooler_bwd(hb.data_ptr(), H, None, B, 1, H, W.data_ptr(), b.data_ptr(), dp.data_ptr(), dpre.data_ptr(),
                                       dwb.data_ptr(), dwb[H * H:].data_ptr(), dh0.data_ptr(), stream()) == 0
    torch.cuda.synchronize()
    return dwb, dh0
