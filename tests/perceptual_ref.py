"""fp64 yardstick of the perceptual term's backward (PerceptualLoss(differentiable=True)), from the oracle's layer list
and torch's CPU ops alone.

``routed_backward`` differentiates ``mean |f_a - f_b|`` with respect to the 1-channel image whose *stored* activations
it is given: every decision of the chain (the L1 sign, the ReLU masks, the max-pool argmax) is read from those stored
maps, the arithmetic (transposed convs) is fp64.  With an fp64 forward's own maps it is torch.autograd's gradient
(tests/test_perceptual_grad_cpu.py pins that); with the native bf16 forward's maps it is the exact gradient through that
stored forward, the thing the kernels compute up to the bf16 rounding of each inter-layer gradient (``round``).
"""
import torch
import torch.nn.functional as F

from oracle import climsr_ref as ref


def bf16_round(t: torch.Tensor) -> torch.Tensor:
    return t.float().bfloat16().to(t.dtype)


def forward_acts(params, x3):
    """The oracle's VGG19[:35] forward (ref.vgg19_features) that also returns what the native forward stores: each
    conv's output after its ReLU (conv5_4: none) and before its pool, NCHW."""
    acts, out = [], x3
    for idx, _cin, _cout, relu, pool in ref.vgg19_layers():
        out = F.conv2d(out, params[f"loss_network.{idx}.weight"], params[f"loss_network.{idx}.bias"], padding=1)
        if relu:
            out = F.relu(out)
        acts.append(out)
        if pool:
            out = F.max_pool2d(out, 2, 2)
    return acts, out


def routed_backward(params64, acts, f_a, f_b, round=None):
    """d mean|f_a - f_b| / d image of the half whose 16 stored maps are ``acts`` (NCHW, as forward_acts returns them) and
    whose conv5_4 features are f_a; [n,1,h,w] fp64.  round: applied to the gradient after each layer (bf16_round models
    the native chain).  For the other argument of the loss swap f_a and f_b."""
    layers = ref.vgg19_layers()
    g = torch.sign(f_a.double() - f_b.double())
    numel = f_a.numel()
    for k in range(len(layers) - 1, -1, -1):
        idx, _cin, _cout, relu, pool = layers[k]
        act = acts[k].double()
        if pool:  # torch's CPU rule: the first maximum of the window in row-major order
            _pooled, ind = F.max_pool2d(act, 2, 2, return_indices=True)
            g = F.max_unpool2d(g, ind, 2, 2, output_size=act.shape[-2:])
        if relu:
            g = g * (act > 0)
        g = F.conv_transpose2d(g, params64[f"loss_network.{idx}.weight"].double(), padding=1)
        if round is not None:
            g = round(g)
    return g.sum(1, keepdim=True) / numel
