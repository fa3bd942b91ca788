"""vd_hallucinator_bwd in the ordered mode (vd_set_deterministic): the hallucinator's weight and bias gradient, which both default
forms close with one fp32 atomic per workgroup in whatever order the workgroups finish, come from ONE workgroup per parameter
job -- the same bits on every call -- and are torch's own fp64 Conv3d gradient within the bound the fixed order allows."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _grads(net, static, dynamic, g_out):
    for p in net.parameters():
        p.grad = None
    dyn = dynamic.clone().requires_grad_(True)
    net(static, dyn).backward(g_out)
    return [net.encoder.weight.grad.clone(), net.encoder.bias.grad.clone(), dyn.grad.clone()]


@pytest.mark.parametrize("n,T,H,W", [(6, 8, 64, 64), (3, 4, 19, 37)])
def test_the_ordered_form_repeats_its_bits_and_is_the_gradient(n, T, H, W):
    from video_distillation_amd import hip, utils
    g = torch.Generator().manual_seed(n + H)
    static, dynamic = torch.randn(n, 3, H, W, generator=g).cuda(), torch.randn(n, T, 1, H, W, generator=g).cuda()
    g_out = torch.randn(n, T, 3, H, W, generator=g).cuda()
    torch.manual_seed(1)
    net = utils.Conv3DNet().cuda()
    # torch's own Conv3d on the concatenated input, in fp64
    ref = torch.nn.Conv3d(4, 3, 3, padding=1).cuda().double()
    ref.load_state_dict({k: v.double() for k, v in net.encoder.state_dict().items()})
    x = torch.cat([static[:, :, None].expand(-1, -1, T, -1, -1), dynamic.permute(0, 2, 1, 3, 4)], 1).double()
    ref(x).backward(g_out.permute(0, 2, 1, 3, 4).double())
    want_w, want_b = ref.weight.grad, ref.bias.grad
    before = hip.set_deterministic(False)
    try:
        loose = _grads(net, static, dynamic, g_out)
        hip.set_deterministic(True)
        first = _grads(net, static, dynamic, g_out)
        for _ in range(3):
            again = _grads(net, static, dynamic, g_out)
            assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(first, again))
    finally:
        hip.set_deterministic(before)
    # The bound.  One workgroup of 256 threads per job: a thread adds the products of its ceil(n H W / 256) pixel columns frame by
    # frame (for the static channels: the temporal sum of the upstream gradient first, T additions, then one product per column),
    # then 6 wave steps and 3 additions over the four waves, then one add onto zero.  With the product's own rounding no term
    # passes through more than a = ceil(n H W / 256) * T + T + 11 roundings of 2^-24, so per element
    # |got - fp64| <= a * 2^-24 * sum|terms|, and sum|terms| is the same Conv3d gradient on the absolute values.
    absref = torch.nn.Conv3d(4, 3, 3, padding=1).cuda().double()
    absref(x.abs()).backward(g_out.permute(0, 2, 1, 3, 4).double().abs())
    a = -(-(n * H * W) // 256) * T + T + 11
    for name, got, want, mag in (("g_w", first[0], want_w, absref.weight.grad), ("g_b", first[1], want_b, absref.bias.grad)):
        err, bound = (got.double() - want).abs(), a * 2.0 ** -24 * mag
        print("%s: a = %d, worst error %.3f of its bound" % (name, a, float((err / bound).max())))
        assert bool((err <= bound).all()), name
    assert torch.equal(first[2], loose[2])          # the data half is the same kernel in both modes
