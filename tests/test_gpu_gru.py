"""The four GRU step kernels of csrc/gru.hip (gru_step_kernel: fp32; gru_step_v2_kernel: split-f16, B > 64; gru_step_small_kernel<1> / <2>:
split-f16, B <= 32 / <= 64) through ops.gru_step, against the fp64 step of oracle/pmce_oracle.py (itself pinned to torch.nn.GRU on the host:
tests/test_gru_oracle_host.py): both forms, two directions, the model's strides, batch tails, other H, saturated gates, non-finite rows, the
recurrence as model.cpp's gru_layer lays it out, and the GRU inside the model.

Inputs follow test_gru_step_small_batch_equals_v2: a seeded torch.Generator, whh ~ N(0, 1/H) with one row per direction scaled by 300 (the
per-row scales of the packed weight matter), bhh ~ 0.1 N, h = tanh(N), gi ~ N.

Bounds.  A single step: BOUND = 5e-6 max-abs against fp64 (what test_gru_step_small_batch_equals_v2 holds the split form to; the plain fp32
step on the CPU is 4-7e-7 from fp64 on these inputs).  A recurrence: ten times the error of the plain fp32 recurrence on the CPU for the same
inputs, computed inside the test, and never more than 5e-5 (test_gru_all_steps_fixture's bound).  "Same bits" is torch.equal.

Measured on an MI355X (max-abs against fp64; `-s` prints them on every run):
  (a) sweep B = 1 ... 129, H = 1024        fp32 form 5.8e-7, split form 4.8e-7                 bound 5e-6
  (c) direction plumbing, B = 5 / 40 / 70  fp32 form 1.0e-6, split form 7.0e-7                 bound 5e-6
  (d) first step                           both forms 1.0e-7                                   bound 5e-6
  (e) H = 256 / 512 / 768                  fp32 form 3.0e-7 / 3.5e-7 / 5.1e-7, split form 2.7e-7 / 3.0e-7 / 3.1e-7   bound 5e-6
  (f) saturated gates, B = 40 / 70         fp32 form 4.1e-7, split form 4.3e-7                 bound 5e-6
  (g) the units fed +inf                   both forms 1.0e-7                                   bound 5e-6
  (h) one clip at rows 0 / 8 / 16 / 24     fp32 form 3.4e-7, split form 2.0e-7                 bound 5e-6
  (i) 16 steps, H = 1024 B = 40            fp32 form 1.6e-6, split form 9.6e-7 (plain fp32 9.2e-7: bound 9.2e-6)
      16 steps, H = 256 B = 70             fp32 form 2.9e-6, split form 2.8e-6 (plain fp32 2.1e-6: bound 2.1e-5)
  (j) model, B = 3 / 40 / 70, default      Y0 6.9e-7 / 9.6e-7 / 9.6e-7 (bound 1.8e-6 / 2.4e-6 / 2.4e-6), Y1 5.7e-7 / 6.9e-7 / 6.9e-7 (bound 1.8e-6 / 2.0e-6 / 2.0e-6)
      model, B = 3 / 40 / 70, f32          Y0 8.1e-7 / 8.4e-7 / 8.4e-7,                                   Y1 5.7e-7 / 8.1e-7 / 8.1e-7 (the same bounds)
(b), and every "same bits" claim of (c), (d), (g) and (h), hold exactly.
"""
import pytest
import torch

from conftest import cached_state_dict
from test_gpu_ops import T, _pmce17, dev, maxabs

pytestmark = pytest.mark.gpu

BOUND = 5e-6            # one step against fp64
RECURRENCE_CAP = 5e-5   # a recurrence, whatever the plain fp32 one does
SENT = 7.0              # |h'| <= 1: no output is ever the sentinel
PAD = 8                 # sentinel rows in front of and behind the rows a call may write
SWEEP = (1, 31, 32, 33, 63, 64, 65, 96, 127, 128, 129)
FORMS = ("f32", "split")


class Case:
    """Two directions' weights, gi [rows, 6H] and h [rows, 2H] laid out as the model's layer 0 has them, and the fp64 step per direction."""

    def __init__(self, H, rows, seed, outliers, scale1=1.0, bias1=0.1):
        from oracle import pmce_oracle as O
        g = torch.Generator().manual_seed(seed)
        self.H, self.rows = H, rows
        self.whh, self.bhh = [], []
        for d in range(2):
            w = torch.randn(3 * H, H, generator=g) * H ** -0.5 * (1.0, scale1)[d]
            if outliers[d] is not None:
                w[outliers[d]] *= 300.0
            self.whh.append(w)
            self.bhh.append(torch.randn(3 * H, generator=g) * (0.1, bias1)[d])
        self.gi = torch.randn(rows, 6 * H, generator=g)
        self.h = torch.tanh(torch.randn(rows, 2 * H, generator=g))
        self.O = O
        self.outliers = outliers
        self.ref = self.reference(self.gi, self.h)
        self._dev = None
        assert self.condition(self.gi, self.h) < CONDITION, "the fixture is ill-conditioned: choose another seed"

    def condition(self, gi, h):
        """The largest |dh'/dgh_r| * sum_k |w_k h_k| over the rows, at the outlier units (fp64): what a relative error of the dot product, in units
        of the sum of its terms' magnitudes, is multiplied by on its way to h'."""
        H, worst = self.H, 0.0
        for d, u in enumerate(self.outliers):
            if u is None:
                continue
            x, hh = gi[:, 3 * H * d:3 * H * (d + 1)].double(), h[:, H * d:H * (d + 1)].double()
            gh = hh @ self.whh[d].double().T + self.bhh[d].double()
            r, z = torch.sigmoid(x[:, u] + gh[:, u]), torch.sigmoid(x[:, H + u] + gh[:, H + u])
            n = torch.tanh(x[:, 2 * H + u] + r * gh[:, 2 * H + u])
            sens = ((1 - z) * (1 - n * n) * gh[:, 2 * H + u] * r * (1 - r)).abs()
            worst = max(worst, float((sens * (hh.abs() @ self.whh[d][u].double().abs())).max()))
        return worst

    def reference(self, gi, h, dtype=torch.float64):
        """[rows, 2H]: the step of both directions (h None: the first step)."""
        H = self.H
        return torch.cat([self.O.gru_step(gi[:, 3 * H * d:3 * H * (d + 1)], self.whh[d], self.bhh[d],
                                          None if h is None else h[:, H * d:H * (d + 1)], dtype) for d in range(2)], 1)

    def weights(self):
        if self._dev is None:
            self._dev = [w.to(dev()) for w in self.whh], [b.to(dev()) for b in self.bhh]
        return self._dev


_CASES, _RUNS = {}, {}


# The outlier rows are reset-gate rows, as in test_gru_step_small_batch_equals_v2 (row 5).  Their gh_r is a sum of terms of some hundreds, and in a
# row where it happens to cancel against gi_r the reset gate is in its linear range and h' moves by up to 400 times the dot product's relative
# error (in units of the sum of its terms' magnitudes): at such seeds the PLAIN fp32 step on the CPU is 3e-6 to 6e-6 from fp64, and BOUND, set where
# it is 4.5e-7, would judge the dice and not the kernel.  Every fixture is therefore drawn from the first seed >= 77 at which that factor stays below
# CONDITION in every row (computed in fp64, asserted when the fixture is made): a dot product good to 2^-22 of the sum of its terms' magnitudes - the
# three-product form's design precision - then moves h' by at most 10 * 2.4e-7 = 2.4e-6, half of BOUND.  (An outlier in the update gate is worse: z
# multiplies h - n directly; the plain fp32 step is then 7.7e-6 from fp64.)
CONDITION = 10.0
SEEDS = {(1024, 129): 86, (256, 70): 77, (512, 70): 78, (768, 70): 77}


def case(H, rows=129, seed=None, outliers=None, **kw):
    outliers = (5, 11) if outliers is None else outliers
    seed = SEEDS[(H, rows)] if seed is None else seed
    key = (H, rows, seed, outliers, tuple(sorted(kw.items())))
    if key not in _CASES:
        if len(_CASES) > 3:
            _CASES.clear()
            _RUNS.clear()
        _CASES[key] = Case(H, rows, seed, outliers, **kw)
    return _CASES[key]


def halves(t, w):
    return [t[:, :w], t[:, w:]]


def run(c, B, form, blocked=True, h_prev="both", gi=None, h=None, only=None):
    """One call on the model's layer-0 layout: gi a [B, 6H] buffer, h_prev and out [B, 2H] buffers, direction 1 at columns 3H / H.  `out` is rows
    [PAD, PAD + B) of a sentinel-filled buffer, returned whole.  only = 0 / 1: an ndir = 1 call of that direction alone (1: the model's
    backward-only convention); the other direction's columns must then stay untouched."""
    from pmce_amd import ops
    H, d = c.H, dev()
    GI = (c.gi if gi is None else gi)[:B].to(d)
    Hp = (c.h if h is None else h)[:B].to(d)
    buf = torch.full((B + 2 * PAD, 2 * H), SENT, device=d)
    gis, hps, outs = halves(GI, 3 * H), halves(Hp, H), halves(buf[PAD:PAD + B], H)
    hp = {"both": hps, None: None, "d0": [hps[0], None], "d1": [None, hps[1]]}[h_prev]
    whh, bhh = c.weights()
    if only is None:
        ops.gru_step(gis, whh, bhh, hp, outs, form=form, blocked=blocked)
    elif only == 0:
        ops.gru_step(gis[0], whh[:1], bhh[:1], None if hp is None else hp[0], outs[0], form=form, blocked=blocked)
    else:
        ops.gru_step(gis[1], whh, bhh, None if hp is None else hp[1], outs[1], form=form, blocked=blocked, backward_only=True)
    return buf.cpu()


def live(buf, B):
    return buf[PAD:PAD + B]


def untouched(buf, B):
    return bool((buf[:PAD] == SENT).all()) and bool((buf[PAD + B:] == SENT).all())


def sweep_run(form, B):
    """The runs of (a), shared with (b)."""
    key = (form, B)
    if key not in _RUNS:
        _RUNS[key] = run(case(1024), B, form)
    return _RUNS[key]


# ---- (a) both forms against fp64 over the batch sweep ----------------------------------------------------------------------------------
@pytest.mark.parametrize("B", SWEEP)
@pytest.mark.parametrize("form", FORMS)
def test_step_matches_fp64_over_the_batch_sweep(form, B):
    """ndir = 2 at the model's layer-0 strides, every batch tail of the 32- and 64-row tiles: the live rows within BOUND of fp64 per direction,
    nothing written outside rows [0, B).  Measured, the largest over the sweep: fp32 form 5.8e-7, split form 4.8e-7."""
    c = case(1024)
    buf = sweep_run(form, B)
    out, H = live(buf, B), c.H
    e = [maxabs(out[:, H * d:H * (d + 1)], c.ref[:B, H * d:H * (d + 1)]) for d in range(2)]
    print(f"(a) {form} B = {B}: direction 0 {e[0]:.2e}, direction 1 {e[1]:.2e} against fp64 (bound {BOUND:.0e})")
    assert untouched(buf, B), "rows outside [0, B) were written"
    assert e[0] <= BOUND and e[1] <= BOUND


# ---- (b) the same row index at any B: the same bits ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_same_row_same_bits_at_every_batch_size(form):
    """Row i of every B of the sweep is row i of the B = 129 run, bit for bit: two directions, strided buffers, both forms."""
    big = live(sweep_run(form, 129), 129)
    for B in SWEEP:
        out = live(sweep_run(form, B), B)
        assert torch.equal(out, big[:B]), f"{form} B = {B}: differs from the same rows at B = 129 by {maxabs(out, big[:B]):.2e}"


@pytest.mark.parametrize("B", (1, 33, 65, 129))
def test_blocked_and_row_major_weight_same_bits(B):
    """Split form, two directions packed in one call: the blocked layout (what the model runs) and the row-major one give the same bits."""
    rm = run(case(1024), B, "split", blocked=False)
    assert untouched(rm, B)
    assert torch.equal(rm, sweep_run("split", B))


# ---- (c) direction plumbing ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", (5, 40, 70))
@pytest.mark.parametrize("form", FORMS)
def test_two_directions_equal_two_single_direction_calls(form, B):
    """The ndir = 2 call against direction 0 alone and direction 1 alone through the backward-only convention (direction 1's rows of the stacked
    weight, the scale table + 3H), against direction 1's weight on its own (split: packed alone, ops.gru_step_split), all bit for bit.  The two
    directions differ visibly (direction 1: twice the weight scale, three times the bias scale) and ONLY direction 1 has the outlier row: a
    swapped or unshifted scale table fails."""
    from pmce_amd import ops
    c = case(1024, rows=70, seed=77, outliers=(None, 7), scale1=2.0, bias1=0.3)
    H, d = c.H, dev()
    both = run(c, B, form)
    d0, d1 = run(c, B, form, only=0), run(c, B, form, only=1)
    assert untouched(both, B) and untouched(d0, B) and untouched(d1, B)
    assert bool((live(d0, B)[:, H:] == SENT).all()) and bool((live(d1, B)[:, :H] == SENT).all()), "a single-direction call wrote the other direction's columns"
    assert torch.equal(live(both, B)[:, :H], live(d0, B)[:, :H]), "direction 0 of the ndir = 2 call differs from the ndir = 1 call"
    assert torch.equal(live(both, B)[:, H:], live(d1, B)[:, H:]), "direction 1 of the ndir = 2 call differs from the backward-only call"
    gi1, h1 = c.gi[:B, 3 * H:].contiguous().to(d), c.h[:B, H:].contiguous().to(d)
    whh, bhh = c.weights()
    alone = torch.full((B, H), SENT, device=d)
    ops.gru_step(gi1, whh[1:], bhh[1:], h1, alone, form=form)                # contiguous operands, the direction's weight alone
    assert torch.equal(alone.cpu(), live(both, B)[:, H:])
    if form == "split":
        assert torch.equal(ops.gru_step_split(gi1, whh[1], bhh[1], h1).cpu(), live(both, B)[:, H:])
    e = maxabs(live(both, B), c.ref[:B])
    print(f"(c) {form} B = {B}: ndir = 2 == two ndir = 1 calls == direction 1 alone, bit for bit; {e:.2e} against fp64")
    assert e <= BOUND


# ---- (d) the first step, and a first step in one direction only -------------------------------------------------------------------------------
@pytest.mark.parametrize("B", (7, 40, 70))
@pytest.mark.parametrize("form", FORMS)
def test_first_step_and_mixed_first_step(form, B):
    """h_prev = None equals h_prev = zeros bit for bit in both forms (split: the planes of 0 are 0 and every product with them is +0, so gh is
    exactly +0 as when the loop is skipped); h_prev given for one direction only equals the two separate calls (the `if (hp)` branch with its
    barriers is uniform per workgroup: a workgroup belongs to one direction)."""
    c = case(1024)
    none = run(c, B, form, h_prev=None)
    zeros = run(c, B, form, h=torch.zeros_like(c.h))
    assert untouched(none, B) and torch.equal(none, zeros)
    e = maxabs(live(none, B), c.reference(c.gi, None)[:B])
    print(f"(d) {form} B = {B}: first step {e:.2e} against fp64")
    assert e <= BOUND
    H = c.H
    full = live(sweep_run(form, B) if B in SWEEP else run(c, B, form), B)
    for which, with_h in (("d0", 0), ("d1", 1)):
        mixed = run(c, B, form, h_prev=which)
        assert untouched(mixed, B)
        cols = lambda t, dd: t[:, H * dd:H * (dd + 1)]      # noqa: E731
        assert torch.equal(cols(live(mixed, B), with_h), cols(full, with_h)), f"h_prev for direction {with_h} only: that direction differs"
        assert torch.equal(cols(live(mixed, B), 1 - with_h), cols(live(none, B), 1 - with_h)), f"h_prev for direction {with_h} only: the other differs"
        alone = run(c, B, form, h_prev=which, only=with_h)
        assert torch.equal(cols(live(alone, B), with_h), cols(live(mixed, B), with_h))


# ---- (e) other H -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", (3, 40, 70))
@pytest.mark.parametrize("H", (256, 512, 768))
@pytest.mark.parametrize("form", FORMS)
def test_other_hidden_sizes(form, H, B):
    """H = 256 (four k-tiles per K-quarter: the small kernels' prologue issues them all, v2's ring of three wraps once), 512, 768; one batch
    each of the NT = 1, NT = 2 and v2 kernels."""
    c = case(H, rows=70)
    buf = run(c, B, form)
    e = maxabs(live(buf, B), c.ref[:B])
    print(f"(e) {form} H = {H} B = {B}: {e:.2e} against fp64")
    assert untouched(buf, B)
    assert e <= BOUND
    if form == "split":
        assert torch.equal(run(c, B, form, blocked=False), buf)


# ---- (f) saturated gates ----------------------------------------------------------------------------------------------------------------------
def saturated_gi(c):
    """Column patterns over the units u of both directions: reset gate +30 / -30 at u % 4 == 0 / 1, update gate +100 / -100 at u % 3 == 0 / 1
    (expf overflows for -100, underflows for +100), candidate pre-activations scaled by 40 (tanh saturated)."""
    H = c.H
    gi = c.gi.clone()
    u = torch.arange(H)
    zp, zm = torch.zeros(6 * H, dtype=torch.bool), torch.zeros(6 * H, dtype=torch.bool)
    for d in range(2):
        o = 3 * H * d
        gi[:, o + u[u % 4 == 0]] = 30.0
        gi[:, o + u[u % 4 == 1]] = -30.0
        gi[:, o + H + u[u % 3 == 0]] = 100.0
        gi[:, o + H + u[u % 3 == 1]] = -100.0
        gi[:, o + 2 * H:o + 3 * H] *= 40.0
        zp[o + H + u[u % 3 == 0]] = True
        zm[o + H + u[u % 3 == 1]] = True
    # the masks as columns of the [rows, 2H] output
    sel = lambda m: torch.cat([m[H:2 * H], m[4 * H:5 * H]])      # noqa: E731
    return gi, sel(zp), sel(zm)


@pytest.mark.parametrize("B", (40, 70))
@pytest.mark.parametrize("form", FORMS)
def test_saturated_gates(form, B):
    """Every output finite and within BOUND of fp64; z = 1 exactly (gi_z = +100) keeps h bit for bit; z = 0 exactly (gi_z = -100) gives n."""
    c = case(1024)
    H = c.H
    gi, zp, zm = saturated_gi(c)
    assert c.condition(gi, c.h) < CONDITION
    buf = run(c, B, form, gi=gi)
    out = live(buf, B)
    ref = c.reference(gi, c.h)[:B]
    gh_n = torch.cat([c.h[:B, H * d:H * (d + 1)].double() @ c.whh[d][2 * H:].double().T + c.bhh[d][2 * H:].double() for d in range(2)], 1)
    gh_r = torch.cat([c.h[:B, H * d:H * (d + 1)].double() @ c.whh[d][:H].double().T + c.bhh[d][:H].double() for d in range(2)], 1)
    gi_r = torch.cat([gi[:B, 3 * H * d:3 * H * d + H] for d in range(2)], 1).double()
    gi_n = torch.cat([gi[:B, 3 * H * d + 2 * H:3 * H * (d + 1)] for d in range(2)], 1).double()
    n = torch.tanh(gi_n + torch.sigmoid(gi_r + gh_r) * gh_n)
    e, en = maxabs(out, ref), maxabs(out[:, zm], n[:, zm])
    print(f"(f) {form} B = {B}: saturated gates {e:.2e} against fp64, h' against n where z = 0: {en:.2e}")
    assert untouched(buf, B) and bool(torch.isfinite(out).all())
    assert e <= BOUND and en <= BOUND
    assert torch.equal(out[:, zp], c.h[:B][:, zp]), "z = 1 exactly must keep h bit for bit"


# ---- (g) non-finite values stay in their row --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", (33, 65, 70))
@pytest.mark.parametrize("form", FORMS)
def test_nonfinite_values_stay_in_their_row(form, B):
    """The tail rows of a tile are copies of row B - 1: a NaN there must reach no stored row but its own; likewise row 0; +inf in a gi element
    changes that unit's output of that row only (to what the formulas give: sigmoid(inf) = 1, tanh(inf) = 1 - finite) and no other bit."""
    c = case(1024)
    H = c.H
    clean = live(sweep_run(form, B) if B in SWEEP else run(c, B, form), B)
    for row in (B - 1, 0):
        h = c.h.clone()
        h[row, 3] = float("nan")                 # direction 0's h
        h[row, H + 1000] = float("nan")          # direction 1's h
        buf = run(c, B, form, h=h)
        out = live(buf, B)
        others = torch.arange(B) != row
        assert untouched(buf, B)
        assert torch.equal(out[others], clean[others]), f"NaN in h_prev of row {row} changed another row"
        assert bool(torch.isnan(out[row]).all()), f"NaN in h_prev of row {row}: W_hh h is NaN for every unit of both directions"
    mid = B // 2
    gi = c.gi.clone()
    gi[mid, 2 * H + 17] = float("inf")           # direction 0, candidate of unit 17
    gi[mid, 3 * H + H + 40] = float("inf")       # direction 1, update gate of unit 40
    buf = run(c, B, form, gi=gi)
    out = live(buf, B)
    hit = torch.zeros(B, 2 * H, dtype=torch.bool)
    hit[mid, 17] = hit[mid, H + 40] = True
    ref = c.reference(gi, c.h)[:B]
    assert untouched(buf, B) and bool(torch.isfinite(ref).all())
    assert torch.equal(out[~hit], clean[~hit]), "+inf in a gi element changed another output"
    e = maxabs(out[hit], ref[hit])
    print(f"(g) {form} B = {B}: NaN rows stay in their row; the two units fed +inf are {e:.2e} from fp64")
    assert bool(torch.isfinite(out).all()) and e <= BOUND
    assert out[mid, H + 40] == c.h[mid, H + 40]  # z = 1: h kept


# ---- (h) place in the batch ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_place_in_the_batch(form):
    """What holds: the same bits at the same row index whatever B (b), and at rows 32 apart (the same place in a 32-row tile); rounding that depends
    on the row's place in its 32-row tile, because the K-quarter that owns accumulator row r = (row >> 3) & 3 adds the other three to its own
    sum last.  The same clip at rows 0, 8, 16, 24 of a B = 32 batch: each within BOUND of fp64; the count of differing elements is printed.
    Measured: of the 2048 elements of the clip, 282 / 288 / 261 (fp32 form) and 278 / 303 / 279 (split form) differ from row 0's at rows 8 / 16 / 24,
    by at most 1.8e-7; each placement is 2.0e-7 to 3.4e-7 from fp64."""
    c = case(1024)
    H = c.H
    gi, h = c.gi.clone(), c.h.clone()
    places = (0, 8, 16, 24, 32, 64, 96)
    for p in places:
        gi[p], h[p] = c.gi[100], c.h[100]
    out32 = live(run(c, 32, form, gi=gi, h=h), 32)
    out128 = live(run(c, 128, form, gi=gi, h=h), 128)
    ref = c.ref[100]
    errs = [maxabs(out32[p], ref) for p in places[:4]]
    differ = [int((out32[p] != out32[0]).sum()) for p in places[1:4]]
    apart = [maxabs(out32[p], out32[0]) for p in places[1:4]]
    print(f"(h) {form}: one clip at rows 0 / 8 / 16 / 24 of B = 32: " + " / ".join(f"{e:.2e}" for e in errs) + f" against fp64; of {2 * H} elements "
          + " / ".join(str(n) for n in differ) + " differ from row 0's (by at most " + " / ".join(f"{a:.1e}" for a in apart) + ")")
    assert all(e <= BOUND for e in errs)
    assert torch.equal(out128[:32], out32)
    for p in (32, 64, 96):
        assert torch.equal(out128[p], out128[0]), f"row {p} and row 0 are the same place in a 32-row tile: same bits expected"


# ---- (i) a 16-step recurrence laid out as model.cpp's gru_layer ------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,B", [(1024, 40), (256, 70)])
def test_recurrence_as_the_model_lays_it_out(H, B):
    """Y[T][B][2H], GI[T][B][6H]; direction 0 walks t = 0..15, direction 1 t = 15..0; every step one ndir = 2 call whose h_prev is the neighbouring
    time slab of Y.  All 16 x 2 slabs against the fp64 recurrence; bound: ten times the plain fp32 recurrence's error, at most 5e-5.
    Measured (plain fp32 on the CPU / fp32 form / split form): H = 1024, B = 40: 9.2e-7 / 1.6e-6 / 9.6e-7; H = 256, B = 70: 2.1e-6 / 2.9e-6 / 2.8e-6."""
    from pmce_amd import ops
    Tn = 16
    c = case(H, rows=70) if H != 1024 else case(1024)
    g = torch.Generator().manual_seed(80)
    GI = torch.randn(Tn, B, 6 * H, generator=g)

    def cpu(dtype):
        Y = torch.zeros(Tn, B, 2 * H, dtype=dtype)
        for d in range(2):
            hcur = None
            for s in range(Tn):
                t = s if d == 0 else Tn - 1 - s
                hcur = c.O.gru_step(GI[t][:, 3 * H * d:3 * H * (d + 1)], c.whh[d], c.bhh[d], hcur, dtype)
                Y[t][:, H * d:H * (d + 1)] = hcur
        return Y

    ref, plain = cpu(torch.float64), cpu(torch.float32)
    e32 = maxabs(plain, ref)
    bound = min(10 * e32, RECURRENCE_CAP)
    whh, bhh = c.weights()
    GId = GI.to(dev())
    errs = {}
    for form in FORMS:
        Y = torch.full((Tn + 2, B, 2 * H), SENT, device=dev())      # a sentinel slab in front and behind
        Yt = Y[1:Tn + 1]
        for s in range(Tn):
            tf, tb = s, Tn - 1 - s
            hp = None if s == 0 else [Yt[tf - 1][:, :H], Yt[tb + 1][:, H:]]
            ops.gru_step([GId[tf][:, :3 * H], GId[tb][:, 3 * H:]], whh, bhh, hp, [Yt[tf][:, :H], Yt[tb][:, H:]], form=form)
        Y = Y.cpu()
        assert bool((Y[0] == SENT).all()) and bool((Y[-1] == SENT).all())
        errs[form] = maxabs(Y[1:Tn + 1], ref)
    print(f"(i) H = {H} B = {B}, 16 steps x 2 directions against fp64: plain fp32 on the CPU {e32:.2e}, fp32 form {errs['f32']:.2e}, "
          f"split form {errs['split']:.2e} (bound {bound:.2e})")
    for form in FORMS:
        assert errs[form] <= bound, form


# ---- (j) inside the model ---------------------------------------------------------------------------------------------------------------------------
_ORACLE = {}


def model_oracle(B):
    """fp64 and plain fp32 GRU of the model's synthetic weights on B synthetic clips, once per B: (top fp64, layer 0 fp64, top fp32, layer 0 fp32)."""
    from oracle import pmce_oracle as O
    from pmce_amd import synth
    if B not in _ORACLE:
        sd = cached_state_dict(17, 256)
        _, feats = synth.make_inputs(B, 17, 23)
        x = T(feats).permute(1, 0, 2).contiguous()
        with torch.no_grad():
            _ORACLE[B] = O.gru_bidir2(x.double(), sd, "pose_mesh_coevo.gru_cur", torch.float64, return_layer0=True) + \
                O.gru_bidir2(x, sd, "pose_mesh_coevo.gru_cur", torch.float32, return_layer0=True)
    return _ORACLE[B]


@pytest.mark.parametrize("B", (3, 40, 70))
@pytest.mark.parametrize("mode", ("default", "f32"))
def test_gru_inside_the_model(mode, B):
    """J = 17, C = 256: all of layer 0's output Y0 (16 steps x 2 directions), the steps of the pruned layer 1 that are computed (forward t <= 8,
    backward t >= 8) and g = y[8] against the fp64 oracle, at batches that take the NT = 1, NT = 2 and v2 kernels (default mode) and the fp32
    kernel with and without a tail (f32 mode), where the time-major strides are real.  Bound: ten times the plain fp32 oracle's error on the same
    rows, at most 5e-5.  Measured: Y0 6.9e-7 to 9.6e-7 (plain fp32 1.8e-7 to 2.4e-7, so 3.5 to 4.6 times it), Y1's steps 5.7e-7 to
    8.1e-7 and g 3.9e-7 to 6.9e-7 (plain fp32 1.8e-7 to 2.0e-7), in both modes."""
    from pmce_amd import synth
    top, l0, top32, l032 = model_oracle(B)
    model = _pmce17()
    p2d, feats = synth.make_inputs(B, 17, 23)
    model.set_gemm_mode(None if mode == "default" else "f32")
    try:
        model(T(p2d).to(dev()), T(feats).to(dev()))
        torch.cuda.synchronize()
        eng = model._engine
        y0 = eng.intermediate("Y0", B, (16, B, 2048)).cpu()
        y1 = eng.intermediate("Y1", B, (16, B, 2048)).cpu()
        g = eng.intermediate("g", B, (B, 2048)).cpu()
    finally:
        model.set_gemm_mode(None)
    parts = lambda y: (y[:9, :, :1024], y[8:, :, 1024:])      # noqa: E731  (the pruned steps are unset: never read)
    e32_0 = maxabs(l032, l0)
    e32_1 = max(maxabs(a, b) for a, b in zip(parts(top32), parts(top)))
    e0 = maxabs(y0, l0)
    e1 = max(maxabs(a, b) for a, b in zip(parts(y1), parts(top)))
    eg = maxabs(g, top[8])
    b0, b1 = min(10 * e32_0, RECURRENCE_CAP), min(10 * e32_1, RECURRENCE_CAP)
    print(f"(j) {mode} B = {B}: Y0 {e0:.2e} (plain fp32 {e32_0:.2e}, bound {b0:.2e}); Y1's computed steps {e1:.2e}, g = y[8] {eg:.2e} "
          f"(plain fp32 {e32_1:.2e}, bound {b1:.2e})")
    assert torch.equal(g, y1[8])
    assert e0 <= b0 and e1 <= b1 and eg <= b1
