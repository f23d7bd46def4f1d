"""Attention operands at the extremes of the score distribution, shared by the emulated and the GPU attention tests (a
plain helper module).  Every kernel with an online softmax keeps a running maximum, rescales its running state when the
maximum moves, and (csrc/attention.hip, csrc/spatial_attn.hip) skips the rescale when no lane's maximum moved: a
Gaussian input with one spiked key in the first tile takes the same few paths in every test.  The cases here put the
dominant key in every position a code path depends on -- and the bar compares with what the reference's own fp32
operator sequence loses on the same input, so that a case which is hard for any fp32 softmax is not held against the
kernel."""
import torch

HD = 64   # head width of the transformer's attention


def _rnd(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def spike_positions(T):
    """first key tile | last key of key half 0 | first key of key half 1 | last tile (the loop's NEXT = false instance)"""
    return [5, T // 2 - 1, T // 2, T - 1]


def cases(B, T, H, seed=0):
    """yields (name, q, k, v): fp32 [B*T, 64*H] each, built from Gaussian q, k * 1.2 and v unless the case says otherwise"""
    C = HD * H

    def base():
        return _rnd(B * T, C, seed=seed + 1), _rnd(B * T, C, seed=seed + 2) * 1.2, _rnd(B * T, C, seed=seed + 3)

    for p in spike_positions(T):
        q, k, v = base()
        k.view(B, T, C)[:, p] *= 8.0
        yield f'spike@{p}', q, k, v
    # scores that rise with the key index: the maximum of every row moves in every tile; falling: it never moves after
    # a key half's first tile, so every later tile of both halves takes the skip branch
    for name, c in (('rise', torch.linspace(0.01, 3.0, T)), ('fall', torch.linspace(0.01, 3.0, T).flip(0))):
        q, k, v = base()
        k = c.view(1, T, 1).expand(B, T, C).reshape(B * T, C).contiguous()
        yield name, q.abs(), k, v
    # every query has its own dominant key: the lanes of a wave move their maxima in different tiles
    q, k, v = base()
    src = (37 * torch.arange(T)) % T
    q = (3.0 * k.view(B, T, C)[:, src]).reshape(B * T, C).contiguous()
    yield 'scattered', q, k, v
    # one key far below the rest: its p underflows to 0 and nothing else may change
    q, k, v = base()
    q = q.abs()
    k.view(B, T, C)[:, T - 2] = -30.0 * float(q.mean())
    yield 'one_below', q, k, v
    # uniform softmax: the result is the mean of v over the keys
    q, k, v = base()
    yield 'uniform_q0', torch.zeros_like(q), k, v
    q, k, v = base()
    k = k.view(B, T, C)[:, :1].expand(B, T, C).reshape(B * T, C).contiguous()
    yield 'uniform_k', q, k, v
    q, k, v = base()
    yield 'onehot', q * 12.0, k * 12.0, v
    # alpha underflows to exactly 0 and the exp2 arguments go below -126
    q, k, v = base()
    yield 'extreme', q * 40.0, k * 40.0, v
    q, k, v = base()
    yield 'large_v', q, k, v * 3000.0


UNIFORM = ('uniform_q0', 'uniform_k')


def heads(t, B, T, H):
    return t.view(B, T, H, HD).permute(0, 2, 1, 3)


def reference_fp64(q, k, v, B, T, H):
    qh, kh, vh = (heads(t.double(), B, T, H) for t in (q, k, v))
    p = torch.softmax(qh @ kh.transpose(2, 3) / 8.0, dim=3)
    return (p @ vh).permute(0, 2, 1, 3).reshape(B * T, H * HD)


def eager_fp32(q, k, v, B, T, H):
    """the reference model's own operator sequence (CausalSelfAttention.forward) in fp32, on the tensors' device"""
    qh, kh, vh = (heads(t, B, T, H) for t in (q, k, v))
    att = torch.softmax((qh @ kh.transpose(-2, -1)) * (1.0 / 8.0), dim=-1)
    return (att @ vh).transpose(1, 2).contiguous().view(B * T, H * HD)


def v_mean(v, B, T, H):
    """what a uniform softmax gives: the per-image, per-head mean of v over the keys, at every query"""
    return v.double().view(B, T, H * HD).mean(dim=1, keepdim=True).expand(B, T, H * HD).reshape(B * T, H * HD)


def allowed(err_eager, v):
    """twice the eager fp32 sequence's own error + 5e-6 of the value scale (tests/test_gpu_split.py: es < 5e-6 + 2 e32)"""
    return 2.0 * err_eager + 5e-6 * max(1.0, float(v.abs().max()))


def bar(err, err_eager, v):
    return err <= allowed(err_eager, v)


def max_err(y, ref):
    return (y.detach().cpu().double() - ref).abs().max().item()


def spatial_cases(n_img, N, C, seed=0):
    """the spike / rise / fall / onehot / uniform_q0 families for one head of width C (the decoder's AttnBlock; scores are
    q.k / sqrt(C)); yields (name, qkv [n_img * N, 3C])"""

    def base():
        return [_rnd(n_img * N, C, seed=seed + 11 + i) * 0.7 for i in range(3)]

    for p in (N // 2 - 1, N // 2, N - 1):
        q, k, v = base()
        k.view(n_img, N, C)[:, p] *= 8.0
        yield f'spike@{p}', torch.cat([q, k, v], dim=1)
    for name, c in (('rise', torch.linspace(0.01, 3.0, N)), ('fall', torch.linspace(0.01, 3.0, N).flip(0))):
        q, k, v = base()
        k = c.view(1, N, 1).expand(n_img, N, C).reshape(n_img * N, C)
        yield name, torch.cat([q.abs(), k, v], dim=1)
    q, k, v = base()
    yield 'onehot', torch.cat([q * 12.0, k * 12.0, v], dim=1)
    q, k, v = base()
    yield 'uniform_q0', torch.cat([torch.zeros_like(q), k, v], dim=1)
