"""Reference forward pass of the bf16 policy engine's numerical contract (include/gaq.h GAQ_POLICY_ENGINE_MFMA_BF16), in fp64 torch:
the weights and every layer input are rounded to bf16 (round to nearest even) explicitly, on the fp32 bits; sums, activations and the
output tanh run in fp64.  The device sums in fp32 in the matrix core's order, so a hidden unit near a bf16 rounding boundary may round
the other way there: the tests compare with two tolerances."""
import torch


def bf16_round(x):
    """fp32 tensor -> fp32 tensor of the nearest bf16 values (ties to even), computed on the bits; NaN stays NaN, +-inf and +-0 stay."""
    x = x.to(torch.float32).contiguous()
    u = x.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    r = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    r = torch.where(torch.isnan(x), (u | 0x00400000) & 0xFFFF0000, r)       # a NaN keeps its sign and stays quiet
    r = torch.where(r >= 0x80000000, r - (1 << 32), r)
    return r.to(torch.int32).view(torch.float32)


def forward(layers, hidden_act, out_tanh, obs):
    """layers = [(W [out, in], b [out]), ...] (fp32, numpy or torch), obs [N, in] fp32 torch -> the 4 outputs [N, 4] in fp64 (before any
    exploration term)."""
    dev = obs.device
    act = torch.tanh if hidden_act == "tanh" else torch.relu
    h = obs.to(torch.float32)
    for k, (W, b) in enumerate(layers):
        W = bf16_round(torch.as_tensor(W, device=dev)).to(torch.float64)
        b = torch.as_tensor(b, device=dev).to(torch.float32).to(torch.float64)
        z = bf16_round(h).to(torch.float64) @ W.T + b
        if k < len(layers) - 1:
            h = act(z).to(torch.float32)
        else:
            h = torch.tanh(z) if out_tanh else z
    return h
