"""The split-f16 number format on the host, for the tests that compare the library's planes against a re-split."""
import torch


def planes(x):
    """[2, M, K] f16 buffer in the library's interleaved layout (isc_seg.A_hi): per row and 32-k block 32 hi then 32 lo."""
    M, K = x.shape
    hi = x.to(torch.float16)
    lo = ((x - hi.float()) * 2048.0).to(torch.float16)
    buf = torch.stack([hi.view(M, K // 32, 32), lo.view(M, K // 32, 32)], dim=2)       # [M, K/32, 2, 32]
    return buf.reshape(2, M, K).contiguous()
