"""Sampled bottom-index refinement, a plain helper module: the fp64 restatement of
t2h_routed_head_sample and the property code of its kernel tests, written once and parametrised by HOW TO LAUNCH
(decode_bands.Env): tests/test_refine_sample_emulated.py runs it on the kernels' source through tests/emu,
tests/test_gpu_refine_sample.py on the hardware.

Every launch goes through the C entry point with out_lists, logp and logits_ws between guard bands pre-filled with
poison (tests/guard_util.py) and the feature rows inside a wider buffer whose 32 pad columns are poison, so every
property below also checks that nothing is written beside the extents and that the pad is never read.

Shapes: 3 heads, Cf = 32, ldf = 3 * 32 + 32; n_class = 37 (tail lanes of the 256-thread class loop), 512 (the
checkpoints' bottom codebook, two classes per thread) or 1024 (four)."""
import ctypes

import torch

import decode_bands as D
import guard_util as G
from text2human_amd._lib import RoutedSampleArgs

N_HEADS, CF = 3, 32
LDF = N_HEADS * CF + 32
P_ONE = 1 << 20
NEAR_TIE = 1e-5     # best and runner-up fp64 scores within this, relative: the row is excused
EXCUSED = 0.01      # at most this share of the rows
TOL = 1e-4          # logp / logits against fp64 (tests/test_gpu_train_forward.py's per-row cross-entropy bound)
DRAW_SEED = 7       # problem(seed): the fp32 restatement against the fp64 one excuses zero rows (checked on the CPU)
FREQ_SEED, FREQ_ROWS = 2024, 4096
GRID_THREADS = 512  # of the Philox tests: far fewer threads than elements, so the counter's high part is exercised


def p_q_of(top_p):
    return 0 if top_p is None else int(round(top_p * P_ONE))


def problem(n, n_class, seed=DRAW_SEED, ties=True, repeat=False):
    """n token rows; ties: per head two identical weight rows + identical bias that dominate the head's first row (an
    exact tie of the two largest logits there, and wherever else they win); repeat: every row is row 0."""
    g = torch.Generator().manual_seed(seed)
    feat = torch.randn(n, N_HEADS * CF, generator=g)
    w = torch.randn(N_HEADS, n_class, CF, generator=g) * 0.3
    b = torch.randn(N_HEADS, n_class, generator=g) * 0.1
    tex = torch.randint(0, N_HEADS, (n, ), generator=g)
    expo = torch.empty(n, n_class).exponential_(generator=g)
    if repeat:
        feat, tex = feat[:1].repeat(n, 1), tex[:1].repeat(n)
    if ties:
        for h in range(N_HEADS):
            if not (tex == h).any():
                continue
            r = int((tex == h).nonzero()[0])
            j1, j2 = 3 + h, n_class - 2 - h
            w[h, j1] = w[h, j2] = 0.5 * feat[r, h * CF:(h + 1) * CF]
            b[h, j2] = b[h, j1]
    return dict(n=n, n_class=n_class, feat=feat.contiguous(), w=w.contiguous(), b=b.contiguous(), tex=tex, expo=expo)


def rows_of(pb, sl):
    """the same problem restricted to token rows sl"""
    out = dict(pb, feat=pb['feat'][sl].contiguous(), tex=pb['tex'][sl].contiguous(), expo=pb['expo'][sl].contiguous())
    out['n'] = out['feat'].shape[0]
    return out


# ---------------------------------------------------------------------------------------------- restatement

def raw64(pb):
    """fp64 logits of every row's own head before the temperature: [n, n_class]"""
    n = pb['n']
    f = pb['feat'].view(n, N_HEADS, CF)[torch.arange(n), pb['tex']].double()
    return torch.einsum('ncf,nf->nc', pb['w'][pb['tex']].double(), f) + pb['b'][pb['tex']].double()


def raw32(pb):
    n = pb['n']
    f = pb['feat'].view(n, N_HEADS, CF)[torch.arange(n), pb['tex']]
    return torch.einsum('ncf,nf->nc', pb['w'][pb['tex']], f) + pb['b'][pb['tex']]


def race(l, expo, mask=None):
    """argmax_j softmax(l)_j / E_j in l's precision, restricted to mask -> (tok [n], near-tie bool [n])"""
    s = torch.softmax(l, 1) / expo.to(l.dtype)
    if mask is not None:
        s = torch.where(mask, s, torch.full_like(s, -1.0))
    top = s.topk(2, dim=1)
    near = (top.values[:, 0] - top.values[:, 1]) <= NEAR_TIE * top.values[:, 0]
    return top.indices[:, 0], near


def logp_of(l, tok):
    return torch.log_softmax(l, 1).gather(1, tok.view(-1, 1)).view(-1)


def assert_tokens(got, want, near, what):
    bad = (got != want) & ~near
    assert int(near.sum()) <= EXCUSED * got.numel(), f'{what}: {int(near.sum())} near-tie rows of {got.numel()}'
    assert not bad.any(), f'{what}: rows {bad.nonzero().flatten().tolist()[:8]} differ from the fp64 restatement'


def binomial_bound_holds(tok, p, what):
    """|frequency_j - p_j| <= 5 sqrt(p_j (1 - p_j) / rows) for every class"""
    rows = tok.numel()
    freq = torch.bincount(tok, minlength=p.numel()).double() / rows
    dev, bound = (freq - p).abs(), 5.0 * torch.sqrt(p * (1 - p) / rows)
    assert (dev <= bound).all(), f'{what}: class {int((dev - bound).argmax())}: |{float(dev.max()):.4f}| beyond the bound'


# ---------------------------------------------------------------------------------------------- launching

class Launch:
    """One t2h_routed_head_sample launch of problem pb.  expo: 'explicit' (pb['expo']), a tensor, or None with
    philox = (seed, offset, grid_threads); table: int32 [B, 3] (per_image_ref.table) with T rows per sample."""

    def __init__(self, env, pb, temp=1.0, top_k=0, top_p_q=0, expo='explicit', philox=None, noise_row0=0, table=None,
                 T=0, want_logp=True, want_ws=True):
        n, n_class = pb['n'], pb['n_class']
        self.env, self.pb = env, pb
        self.fb = D.Buf(env, n, (LDF, ), D.F32, 16, True, cols=(0, N_HEADS * CF)).put(pb['feat'])
        self.tb = D.Buf(env, n, (), torch.int64, 16, True, valid=1).put(pb['tex'])
        self.lb = D.Buf(env, N_HEADS, (n, ), torch.int64, 2, True)
        self.pb_ = D.Buf(env, n, (), D.F32, 16, True)
        self.wb = D.Buf(env, n, (n_class, ), D.F32, 16, True)
        self.keep = [pb['w'].to(env.dev), pb['b'].to(env.dev)]
        a = RoutedSampleArgs()
        a.feat, a.ldf, a.w, a.b, a.tex, a.out_lists = (self.fb.ptr(), LDF, self.keep[0].data_ptr(), self.keep[1].data_ptr(),
                                                       self.tb.ptr(), self.lb.ptr())
        a.n, a.n_heads, a.Cf, a.n_class = n, N_HEADS, CF, n_class
        a.temp, a.top_k, a.top_p_q = temp, top_k, top_p_q
        if expo is not None:
            e = (pb['expo'] if isinstance(expo, str) else expo).to(env.dev).contiguous()
            assert tuple(e.shape) == (n, n_class)
            self.keep.append(e)
            a.expo = e.data_ptr()
        if philox is not None:
            a.philox_seed, a.philox_offset, a.philox_grid_threads = philox
        a.noise_row0 = noise_row0
        a.logp = self.pb_.ptr() if want_logp else None
        a.logits_ws = self.wb.ptr() if want_ws else None
        self.table = table.to(env.dev).contiguous() if table is not None else None
        self.a, self.T = a, T

    def outs(self):
        return [('out_lists', self.lb), ('logp', self.pb_), ('logits_ws', self.wb)]

    def args(self):
        return ctypes.byref(self.a), (self.table.data_ptr() if self.table is not None else None), self.T

    def run(self):
        """launches (bands of the outputs untouched, inputs unwritten) -> self, with lists / tok / logp / ws on the CPU"""
        D.launch_checked(self.env, 'sampler.hip', 't2h_routed_head_sample', self.args(), self.outs(),
                         [('feat', self.fb), ('tex', self.tb)])
        n = self.pb['n']
        self.lists = self.lb.view.cpu().clone()
        self.tok = self.lists[self.pb['tex'], torch.arange(n)]
        off = torch.ones(N_HEADS, n, dtype=torch.bool)
        off[self.pb['tex'], torch.arange(n)] = False
        assert (self.lists[off] == -1).all() and (self.tok >= 0).all() and (self.tok < self.pb['n_class']).all()
        self.logp, self.ws = self.pb_.view.cpu().clone(), self.wb.view.cpu().clone()
        return self

    def rejected(self):
        """the entry point must return an error code and write NOTHING (no byte of any output buffer changes)"""
        for _, b in self.outs():
            b.snap()
        lib = self.env.lib('sampler.hip')
        rc = lib.t2h_routed_head_sample(*self.args(), self.env.stream())
        assert rc != 0
        if self.env.dev != 'cpu':
            torch.cuda.synchronize()
        for what, b in self.outs():
            b.check_unwritten(f'rejected launch: {what}')
        return rc


def argmax_lists(env, pb):
    """t2h_routed_head_argmax on the same buffers' contents -> lists [N_HEADS, n] on the CPU"""
    n = pb['n']
    fb = D.Buf(env, n, (LDF, ), D.F32, 16, True, cols=(0, N_HEADS * CF)).put(pb['feat'])
    tb = D.Buf(env, n, (), torch.int64, 16, True, valid=1).put(pb['tex'])
    lb = D.Buf(env, N_HEADS, (n, ), torch.int64, 2, True)
    wd, bd = pb['w'].to(env.dev), pb['b'].to(env.dev)
    D.launch_checked(env, 'vq.hip', 't2h_routed_head_argmax',
                     (fb.ptr(), LDF, wd.data_ptr(), bd.data_ptr(), tb.ptr(), lb.ptr(), n, N_HEADS, CF, pb['n_class']),
                     [('out_lists', lb)], [('feat', fb), ('tex', tb)])
    return lb.view.cpu().clone()


def philox_expo(env, seed, offset, grid_threads, rows, n_class):
    e = torch.empty(rows, n_class, device=env.dev)
    env.call('sampler.hip', 't2h_philox_exponential_f32', seed, offset, grid_threads, e.data_ptr(), rows * n_class)
    return e


def thresholds(env, ws, top_k, top_p_q, scope=0):
    """t2h_truncation_threshold on logits ws [n, n_class] (CPU tensor) -> theta [n], kept [n] on the CPU"""
    n, n_class = ws.shape
    l = ws.to(env.dev).contiguous()
    theta, kept = torch.empty(n, device=env.dev), torch.empty(n, dtype=torch.int32, device=env.dev)
    env.call('sampler.hip', 't2h_truncation_threshold', l.data_ptr(), n, n_class, top_k, top_p_q, scope, theta.data_ptr(),
             kept.data_ptr())
    return theta.cpu(), kept.cpu()


# ---------------------------------------------------------------------------------------------- properties

def tie_rows(pb):
    """rows whose two largest fp64 logits are exactly equal (the constructed pairs)"""
    top = raw64(pb).topk(2, dim=1)
    return top.values[:, 0] == top.values[:, 1]


def equals_argmax_when_the_noise_says_nothing(env, n, n_class):
    """1: expo of all ones (and top_k = 1 on random expo) == t2h_routed_head_argmax, -1 fill included, lower index of
    an exact tie first.  Under top_k = 1 BOTH classes of an exact tie survive (ties at the threshold all do) and race
    on their own noise: there the token is the tied class with the smaller E, everywhere else the argmax."""
    pb = problem(n, n_class)
    want = argmax_lists(env, pb)
    ties = tie_rows(pb)
    assert int(ties.sum()) >= N_HEADS
    r = torch.arange(n)
    top2 = raw64(pb).topk(2, dim=1).indices
    assert (want[pb['tex'], r][ties] == top2[ties].min(1).values).all()               # the lower index won
    ones = torch.ones(n, n_class)
    for temp in (1.0, 0.7):
        got = Launch(env, pb, temp=temp, expo=ones).run()
        assert torch.equal(got.lists, want), temp
        got = Launch(env, pb, temp=temp, top_k=1).run()
        assert torch.equal(got.lists[:, ~ties], want[:, ~ties]), temp
        e = pb['expo'][r.view(-1, 1), top2]
        winner = torch.where(e[:, 0] <= e[:, 1], top2[:, 0], top2[:, 1])
        assert torch.equal(got.tok[ties], winner[ties]), temp


def the_draw(env, n, n_class):
    """2: token == the fp64 race on every row that is no near-tie; logp / logits within 1e-4 of fp64"""
    pb = problem(n, n_class)
    for temp in (1.0, 0.7):
        l64 = raw64(pb) / temp
        want, near = race(l64, pb['expo'])
        got = Launch(env, pb, temp=temp).run()
        assert_tokens(got.tok, want, near, f'temp {temp}')
        err_l = (got.ws.double() - l64).abs().max().item()
        err_p = (got.logp.double() - logp_of(l64, got.tok)).abs().max().item()
        print(f'n_class {n_class} temp {temp}: max |logits - fp64| {err_l:.2e}, max |logp - fp64| {err_p:.2e}')
        assert err_l <= TOL and err_p <= TOL, (err_l, err_p)
        bare = Launch(env, pb, temp=temp, want_logp=False, want_ws=False).run()                # NULL outputs: skipped
        assert torch.equal(bare.lists, got.lists)
        assert torch.equal(G.bits(bare.wb.whole), G.bits(bare.wb.snapshot))
        assert torch.equal(G.bits(bare.pb_.whole), G.bits(bare.pb_.snapshot))


TRUNC_CASES = [(2, None), (5, None), (64, None), (None, 0.5), (None, 0.9), (5, 0.9), (64, 0.5), (2, 0.5)]


def truncation(env, n, n_class, cases=TRUNC_CASES, temp=0.8, scopes=(0, 1)):
    """3: theta / kept of t2h_truncation_threshold (the workgroup form, scope 0 -- the wave form agrees: the selection
    accumulates integers only) on the kernel's own logits; the token survives, is the restricted race's, and logp stays
    that of the full softmax"""
    pb = problem(n, n_class)
    free = Launch(env, pb, temp=temp).run()
    for top_k, top_p in cases:
        got = Launch(env, pb, temp=temp, top_k=top_k or 0, top_p_q=p_q_of(top_p)).run()
        # logp is the drawn code's log-probability under the FULL softmax: the untruncated call's bits wherever the
        # token is the same, and the full log-softmax of the kernel's logits at the token everywhere
        assert got.ws.numpy().tobytes() == free.ws.numpy().tobytes()
        same = got.tok == free.tok
        assert same.any() and got.logp[same].numpy().tobytes() == free.logp[same].numpy().tobytes()
        assert (got.logp.double() - logp_of(got.ws.double(), got.tok)).abs().max().item() <= TOL
        theta, kept = thresholds(env, got.ws, top_k or 0, p_q_of(top_p), scopes[0])
        for scope in scopes[1:]:
            theta1, kept1 = thresholds(env, got.ws, top_k or 0, p_q_of(top_p), scope)
            assert torch.equal(theta, theta1) and torch.equal(kept, kept1)
        mask = got.ws >= theta.view(-1, 1)
        assert torch.equal(mask.sum(1).int(), kept) and (kept >= 1).all()
        if top_k and top_p is None:
            assert (kept >= min(top_k, n_class)).all() and (kept == min(top_k, n_class)).float().mean() > 0.9
        assert mask[torch.arange(n), got.tok].all(), (top_k, top_p)
        want, near = race(got.ws.double(), pb['expo'], mask)
        assert_tokens(got.tok, want, near, f'top_k {top_k} top_p {top_p}')


def in_kernel_noise(env, n, n_class, seed=0x1234ABCD5, offset=44, rules=(dict(), dict(top_k=5, top_p_q=p_q_of(0.9)))):
    """4: expo == NULL at (seed, offset, grid_threads) == the explicit tensor t2h_philox_exponential_f32 fills with the
    same triple; the last n - 40 rows launched alone with noise_row0 = 40 == those rows of the one launch"""
    pb = problem(n, n_class)
    ph = (seed, offset, GRID_THREADS)
    e = philox_expo(env, *ph, n, n_class)
    for kw in rules:
        want = Launch(env, pb, expo=e.cpu(), **kw).run()
        got = Launch(env, pb, expo=None, philox=ph, **kw).run()
        assert torch.equal(got.lists, want.lists) and got.logp.numpy().tobytes() == want.logp.numpy().tobytes()
        r0 = 40 if n > 40 else n // 2
        part = Launch(env, rows_of(pb, slice(r0, n)), expo=None, philox=ph, noise_row0=r0, **kw).run()
        assert torch.equal(part.lists, got.lists[:, r0:]) and part.ws.numpy().tobytes() == got.ws[r0:].numpy().tobytes()
    assert not torch.equal(got.tok, Launch(env, pb, expo=None, philox=(seed, offset + 4, GRID_THREADS)).run().tok)


PER_SAMPLE_SETS = [(1.0, 0, 0), (0.7, 5, 0), (1.4, 64, p_q_of(0.6))]   # (temp, top_k, top_p_q); image 0: all off


def per_sample_table(env, T, n_class, table_of):
    """5: three samples of T rows with their own rules == the scalar call with each sample's rules, bitwise"""
    pb = problem(3 * T, n_class)
    got = Launch(env, pb, temp=-1.0, top_k=1, top_p_q=1, table=table_of(PER_SAMPLE_SETS), T=T).run()   # (scalars: not read)
    differs = 0
    for i, (temp, k, p_q) in enumerate(PER_SAMPLE_SETS):
        sl = slice(i * T, (i + 1) * T)
        want = Launch(env, pb, temp=temp, top_k=k, top_p_q=p_q).run()
        assert torch.equal(got.lists[:, sl], want.lists[:, sl]), i
        assert got.logp[sl].numpy().tobytes() == want.logp[sl].numpy().tobytes(), i
        assert got.ws[sl].numpy().tobytes() == want.ws[sl].numpy().tobytes(), i
        other = slice(((i + 1) % 3) * T, ((i + 1) % 3 + 1) * T)
        differs += int(got.ws[other].numpy().tobytes() != want.ws[other].numpy().tobytes())
    assert differs == 3                                                       # the table is read per sample


def samples_the_softmax(env, temp, n_class=37):
    """6: one feature row 4096 times, in-kernel noise: every class's frequency within 5 binomial standard deviations"""
    pb = problem(FREQ_ROWS, n_class, seed=FREQ_SEED, ties=False, repeat=True)
    got = Launch(env, pb, temp=temp, expo=None, philox=(FREQ_SEED, 0, GRID_THREADS), want_ws=False).run()
    p = torch.softmax(raw64(pb)[0] / temp, 0)
    binomial_bound_holds(got.tok, p, f'temp {temp}')


def rejected_arguments(env, table_of):
    """7: every rejected argument set returns an error code and writes nothing"""
    pb = problem(12, 37)
    ok = Launch(env, pb).run()
    assert Launch(env, pb, temp=0.0).rejected() and Launch(env, pb, temp=-1.0).rejected()
    assert Launch(env, pb, top_k=-1).rejected() and Launch(env, pb, top_p_q=P_ONE + 1).rejected()
    assert Launch(env, pb, expo=None).rejected()                                       # no noise at all
    assert Launch(env, pb, expo=None, philox=(1, 2, GRID_THREADS)).rejected()          # offset % 4 != 0
    assert Launch(env, pb, expo=None, philox=(1, 4, GRID_THREADS), noise_row0=-1).rejected()
    tbl = table_of(PER_SAMPLE_SETS)
    assert Launch(env, pb, table=tbl, T=5).rejected() and Launch(env, pb, table=tbl, T=0).rejected()   # 5 does not divide 12
    Launch(env, pb, table=tbl, T=4).run()
    for field in ('feat', 'w', 'b', 'tex', 'out_lists'):
        la = Launch(env, pb)
        setattr(la.a, field, None)
        assert la.rejected(), field
    lib = env.lib('sampler.hip')
    assert lib.t2h_routed_head_sample(None, None, 0, env.stream()) != 0
    big = problem(4, 2049, ties=False)
    assert Launch(env, big, top_p_q=p_q_of(0.9)).rejected()                            # top-p: n_class <= 2048
    assert Launch(env, big, table=table_of(PER_SAMPLE_SETS[:2]), T=2).rejected()       # a table: any sample may use it
    Launch(env, big, top_k=7).run()                                                    # top-k alone has no limit
    la = Launch(env, pb)
    la.a.ldf = N_HEADS * CF - 1
    assert la.rejected()
    assert torch.equal(Launch(env, pb).run().lists, ok.lists)
