"""GPU: the two launches of the optimizer step (csrc/vsde_optim.hip: optim_stats_kernel, optim_update_kernel) against the float64
step of tests/optimizer_reference.py, per element: |got - ref| <= c 2^-24 magnitude with the magnitudes and the c of that module
(no bound is relative to a tensor's maximum).

Every case drives ``_hip.optim_step`` with a chunk table built here, in the row layout of ``FusedOptimizerStep._build``
(p, m, v, ema | 0, param | n << 32, goff, group, 0) -- ``test_the_class_builds_the_table_the_tests_mirror`` holds the two together.
p, m, v, the shadow, the gradients and the partial sums each live inside ONE larger NaN-filled buffer, every tensor on a 16-byte
boundary plus the case's offset, with at least 8 sentinel floats between neighbours.  After the step the sentinels and the
gradients (the kernel only reads them) must be bit-identical, every output element within its bound, out[1] exactly 0 or 1,
tstate == [t, t_next]; a second run from the same inputs must give the same bits.

Dispatch coverage (case -> path):

  test_single_chunk        n 1 .. 8                      scalar tail alone (n < 4), one vector trip + tail, two trips
                           n 255 .. 257, 1023 .. 1027    the last thread of a trip idle / full / a tail of 1 and 3 behind 256 x 4 elements
                           n 4093 .. 4096                the fourth trip of every thread with a tail of 1, 2, 3, 0
  test_multi_chunk         n 4097, 8191, 8192, 8193      goff of the second and third record, a last chunk of 1 / 4095 / 4096 / 1
  test_chunk_counts        1, 2, 255, 256, 257, 1000     the strided partial-sum loop of optim_update_kernel: every thread none or one
                                                         partial, thread 0 a second, four per thread; first and last chunk identical bits
  test_alignment           gradient at +0, 1, 2, 3 floats  the per-trip alignment test of optim_stats_kernel (scalar trips) and, with p or
                           p / shadow at +0 or +1          the shadow off by one float too, the ``vec == false`` route of optim_update_kernel
  test_ema_off             ema_weight -1, pointers 0     no shadow buffers at all
  test_full_cross          class x scale x max_norm x t  every input class of the module on the 12-tensor table in three groups
  test_inf_under_a_scale   inf first / tail / misaligned the skipped step: p, m, v bit-unchanged, tstate not advanced, the shadow lerped
  test_three_steps         stage by stage                each step scored from the kernel's own previous state
  test_through_the_class   bucket-view gradients         FusedOptimizerStep with p.grad = flat[k : k + n].view(shape), k % 4 in {1, 2, 3}
"""
import numpy as np
import pytest
import torch

import optimizer_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 8
BUFFERS = ("p", "m", "v", "sh", "g")


def table_rows(ptr, sizes, gids, chunk=R.CHUNK):
    """The chunk records of FusedOptimizerStep._build: ``ptr[k][i]`` is the address of tensor i's first element in p, m, v, sh."""
    rows = []
    for i, (n, gi) in enumerate(zip(sizes, gids)):
        for off in range(0, int(n), chunk):
            cn = min(chunk, int(n) - off)
            rows.append((ptr["p"][i] + 4 * off, ptr["m"][i] + 4 * off, ptr["v"][i] + 4 * off,
                         0 if ptr.get("sh") is None else ptr["sh"][i] + 4 * off, i | (cn << 32), off, int(gi), 0))
    return rows


class Rig:
    """The device buffers and the table of one case; ``off[k]``: floats added to the 16-byte boundary of every tensor in buffer k."""

    def __init__(self, c, off=None):
        from viforsdes_amd import _hip
        assert _hip.optim_chunk_elems() == R.CHUNK
        self.c, off = c, off or {}
        sizes = [int(n) for n in c["sizes"]]
        self.kinds = [k for k in BUFFERS if c[k] is not None]
        self.start, self.host, self.dev, self.mask = {}, {}, {}, {}
        for k in self.kinds:
            starts, cur = [], 0
            for n in sizes:
                s = (cur + GUARD + 3) // 4 * 4 + off.get(k, 0)
                starts.append(s)
                cur = s + n
            host = np.full(cur + GUARD, np.nan, np.float32)
            mask = np.zeros(host.size, bool)
            for s, n, part in zip(starts, sizes, np.split(c[k], np.cumsum(sizes)[:-1])):
                host[s:s + n], mask[s:s + n] = part, True
            self.start[k], self.host[k], self.mask[k] = starts, host, mask
            self.dev[k] = torch.from_numpy(host).to(DEV)
            assert self.dev[k].data_ptr() % 16 == 0
        ptr = {k: [self.dev[k].data_ptr() + 4 * s for s in self.start[k]] for k in self.kinds}
        rows = table_rows(ptr, sizes, c["gids"])
        self.table = torch.tensor(rows, dtype=torch.int64).to(DEV)
        self.grad_ptrs = torch.tensor(ptr["g"], dtype=torch.int64).to(DEV)
        self.groups = torch.from_numpy(np.ascontiguousarray(c["groups"])).to(DEV)
        self.scale = None if c["scale"] is None else torch.tensor(c["scale"], dtype=torch.float32, device=DEV)
        self.n_chunks = len(rows)
        self.partials = torch.full((self.n_chunks + 2 * GUARD,), float("nan"), device=DEV)

    def run(self):
        """One step from the case's inputs -> (flat outputs per kind, whole buffers, out, tstate, partials)."""
        from viforsdes_amd import _hip
        c = self.c
        for k in self.kinds:
            self.dev[k].copy_(torch.from_numpy(self.host[k]))
        self.partials.fill_(float("nan"))
        tstate = torch.tensor([-1.0, c["t"]], dtype=torch.float32, device=DEV)      # the stats kernel publishes t_cur = t_next
        out = torch.full((2,), -1.0, device=DEV)
        _hip.optim_step(self.table, self.grad_ptrs, self.scale, self.partials[GUARD:GUARD + self.n_chunks], tstate, self.groups,
                        c["max_norm"], c["ema_w"], out)
        torch.cuda.synchronize()
        bufs = {k: self.dev[k].cpu().numpy() for k in self.kinds}
        got = {k: bufs[k][self.mask[k]] for k in self.kinds}
        got.setdefault("sh", None)
        return got, bufs, out.cpu().numpy(), tstate.cpu().numpy(), self.partials.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def run_case(c, off=None, label=""):
    """The buffer protocol of the module docstring; returns the kernel's outputs and the worst ratio per kind."""
    rig = Rig(c, off)
    got, bufs, out, tstate, partials = rig.run()
    ref = R.step64(c)
    for k in rig.kinds:                                               # sentinels untouched, gradients only read
        keep = ~rig.mask[k] if k != "g" else np.ones(rig.mask[k].size, bool)
        assert np.array_equal(bits(bufs[k])[keep], bits(rig.host[k])[keep]), (k, "memory outside the tensors changed")
    edge = np.r_[0:GUARD, GUARD + rig.n_chunks:partials.size]
    assert np.isnan(partials[edge]).all() and not np.isnan(partials[GUARD:GUARD + rig.n_chunks]).any()
    assert out[1] in (0.0, 1.0) and bool(out[1]) == ref["found_inf"], out
    assert tstate[0] == c["t"] and tstate[1] == ref["t_next"], tstate
    got["norm"] = float(out[0])
    if ref["found_inf"]:
        assert not np.isfinite(out[0])
        r = {k: R.ratio(got[k], ref[k], ref["mag"][k]) for k in ("p", "m", "v", "sh") if ref[k] is not None}
    else:
        r = R.ratios(c, got, ref)
    print("RATIO " + label + " " + " ".join(f"{k} {v:.4f}" for k, v in r.items()))
    assert R.within(r), r
    again, bufs2, out2, tstate2, partials2 = rig.run()
    for k in rig.kinds:
        assert np.array_equal(bits(bufs2[k]), bits(bufs[k])), (k, "second run differs")
    assert np.array_equal(bits(out2), bits(out)) and np.array_equal(bits(tstate2), bits(tstate))
    got["t_next"] = float(tstate[1])
    return got, r


# ------------------------------------------------------------------------------------------------------------------ shapes
@pytest.mark.parametrize("n", R.SINGLE_CHUNK)
def test_single_chunk(n):
    run_case(R.make_case("general", [n], [n % 3], t=9, scale=1024.0, mode="above"), label=f"n{n}")


@pytest.mark.parametrize("n", R.MULTI_CHUNK)
def test_multi_chunk(n):
    run_case(R.make_case("general", [n], [n % 3], t=9, scale=1024.0, mode="above"), label=f"n{n}")


@pytest.mark.parametrize("k", R.CHUNK_COUNTS)
def test_chunk_counts(k):
    c = R.chunk_count_case(k, t=1, mode="above")
    got, _ = run_case(c, label=f"chunks{k}")
    n = int(c["sizes"][0])
    for key in ("p", "m", "v", "sh"):                                 # every workgroup derives the same clip
        assert np.array_equal(bits(got[key][:n]), bits(got[key][-n:])), key


@pytest.mark.parametrize("other", ["aligned", "p+1", "sh+1"])
@pytest.mark.parametrize("g_off", [0, 1, 2, 3])
def test_alignment(g_off, other):
    off = {"g": g_off}
    if other != "aligned":
        off[other[:-2]] = 1
    run_case(R.make_case("general", R.ALIGN_SIZES, R.ALIGN_GIDS, t=9, scale=1024.0, mode="above"), off, label=f"g+{g_off} {other}")


@pytest.mark.parametrize("g_off", [0, 1])
def test_ema_off(g_off):
    c = R.make_case("general", R.ALIGN_SIZES, R.ALIGN_GIDS, t=1, mode="above", ema_w=-1.0)
    got, r = run_case(c, {"g": g_off}, label="no_ema")
    assert c["sh"] is None and got["sh"] is None and "sh" not in r


# -------------------------------------------------------------------------------------------------------------- full cross
CROSS = [(cls, scale, mode) for cls in R.CLASSES for scale in R.SCALES for mode in R.max_norm_modes(cls)]


@pytest.mark.parametrize("cls,scale,mode", CROSS, ids=lambda v: str(v))
def test_full_cross(cls, scale, mode):
    for t in R.STEPS:
        run_case(R.make_case(cls, R.MIXED_SIZES, R.MIXED_GIDS, t=t, scale=scale, mode=mode), label=f"{cls} t{t}")


# ------------------------------------------------------------------------------------------------------- inf under a scale
@pytest.mark.parametrize("where", ["first", "tail", "misaligned"])
def test_inf_under_a_scale(where):
    c = R.make_case("general", R.ALIGN_SIZES, R.ALIGN_GIDS, t=9, scale=1024.0, mode="above")
    index = {"first": 0, "tail": R.ALIGN_SIZES[0] - 1, "misaligned": R.ALIGN_SIZES[0] + 4097}[where]
    c["g"][index] = np.inf
    got, _ = run_case(c, {"g": 1} if where == "misaligned" else None, label=f"inf {where}")
    for k in ("p", "m", "v"):
        assert np.array_equal(bits(got[k]), bits(c[k])), k
    assert got["t_next"] == 9.0


# ------------------------------------------------------------------------------------------------------------ three steps
def test_three_steps():
    c = R.make_case("general", R.MIXED_SIZES, R.MIXED_GIDS, t=0, scale=1024.0, mode="above")
    for step in range(3):
        got, _ = run_case(c, label=f"step {step}")
        assert got["t_next"] == step + 1
        fresh = R.make_case("general", R.MIXED_SIZES, R.MIXED_GIDS, t=step + 1, scale=1024.0, mode="above" if step else "below", seed=step + 1)
        c = dict(fresh, p=got["p"], m=got["m"], v=got["v"], sh=got["sh"])       # the kernel's own state, a new gradient


# ---------------------------------------------------------------------------------------------------------------- the class
class _Toy(torch.nn.Module):
    SHAPES = {"a": (5,), "b": (33, 7), "c": (4097,), "d": (3, 4101), "theta": (3,)}

    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(0)
        for k, s in self.SHAPES.items():
            x = torch.randn(*s, generator=g)
            self.register_parameter(k, torch.nn.Parameter(torch.sign(x) * (0.1 + x.abs())))


def _class_setup():
    from viforsdes_amd.inference.exponential_moving_average import ExponentialMovingAverage
    from viforsdes_amd.inference.fused_optimizer import FusedOptimizerStep
    model = _Toy().to(DEV)
    hp = lambda row: dict(zip(("lr", "betas", "eps", "weight_decay"), (row[0], (row[1], row[2]), row[3], row[4])))
    opt = torch.optim.AdamW([{"params": [p for n, p in model.named_parameters() if n != "theta"], **hp(R.GROUPS[0])},
                             {"params": [model.theta], **hp(R.GROUPS[1])}])
    ema = ExponentialMovingAverage(model, decay=0.99)
    assert FusedOptimizerStep.usable(opt)
    return model, opt, ema, FusedOptimizerStep(opt, ema, None, max_norm=1.0)


def _bucket_grads(params, seed, mag):
    """Gradients as contiguous views at 4-byte offsets k % 4 in {1, 2, 3} into one flat NaN-filled bucket."""
    total = sum(p.numel() + 8 for p in params)
    flat = torch.full((total,), float("nan"), device=DEV)
    g = torch.Generator().manual_seed(seed)
    cur = 0
    for i, p in enumerate(params):
        k = (cur + 3) // 4 * 4 + 1 + i % 3
        view = flat[k:k + p.numel()].view(p.shape)
        view.copy_(torch.randn(p.shape, generator=g) * mag)
        assert view.is_contiguous() and (view.data_ptr() // 4) % 4 == 1 + i % 3
        p.grad = view
        cur = k + p.numel()
    return flat


def test_the_class_builds_the_table_the_tests_mirror():
    model, opt, ema, fs = _class_setup()
    params = list(model.parameters())
    _bucket_grads(params, 1, 0.01)
    assert fs.step() is not None
    names = [n for n, _ in model.named_parameters()]
    ptr = {"p": [p.data_ptr() for p in params], "m": [opt.state[p]["exp_avg"].data_ptr() for p in params],
           "v": [opt.state[p]["exp_avg_sq"].data_ptr() for p in params], "sh": [ema.shadow[n].data_ptr() for n in names]}
    rows = table_rows(ptr, [p.numel() for p in params], [0, 0, 0, 0, 1])
    assert fs.table.cpu().tolist() == [list(r) for r in rows]
    assert fs.ptr_dev.cpu().tolist() == [p.grad.data_ptr() for p in params]
    assert fs.groups.cpu().numpy().tolist() == R.GROUPS[:2].tolist() and fs.tstate.cpu().tolist() == [0.0, 1.0]


def test_through_the_class():
    model, opt, ema, fs = _class_setup()
    params = list(model.parameters())
    names = [n for n, _ in model.named_parameters()]
    sizes = np.array([p.numel() for p in params])
    gids = np.array([0, 0, 0, 0, 1])
    flat = lambda ts: np.concatenate([t.detach().cpu().numpy().ravel() for t in ts])
    for step in range(2):                                             # norm above, then below max_norm = 1
        _bucket_grads(params, 10 + step, 0.01 if step else 10.0)
        zeros = [torch.zeros_like(p) for p in params]
        c = {"sizes": sizes, "gids": gids, "gid": np.repeat(gids, sizes), "groups": R.GROUPS[:2], "t": float(step), "scale": None,
             "max_norm": 1.0, "ema_w": 1.0 - ema.decay, "p": flat(params), "g": flat([p.grad for p in params]),
             "m": flat([opt.state[p]["exp_avg"] for p in params] if step else zeros),
             "v": flat([opt.state[p]["exp_avg_sq"] for p in params] if step else zeros), "sh": flat([ema.shadow[n] for n in names])}
        norm = fs.step()
        assert norm is not None                                       # the fused route, not the torch sequence
        got = {"p": flat(params), "m": flat([opt.state[p]["exp_avg"] for p in params]),
               "v": flat([opt.state[p]["exp_avg_sq"] for p in params]), "sh": flat([ema.shadow[n] for n in names]), "norm": float(norm)}
        r = R.ratios(c, got)
        print(f"RATIO class step {step} " + " ".join(f"{k} {v:.4f}" for k, v in r.items()))
        assert R.within(r), r
        assert np.array_equal(bits(flat([p.grad for p in params])), bits(c["g"]))
        assert fs.tstate.cpu().tolist() == [float(step), step + 1.0] and ema.fused_step_done
        ema.update()
