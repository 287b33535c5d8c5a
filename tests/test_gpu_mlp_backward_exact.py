"""GPU: dd_mlp_backward's row tiling, block sums and ReLU edge, by identities
that need no measured tolerance.

tests/test_gpu_mlp_backward.py holds the kernel to the float64 restatement
within 4 G 2^-24 S, G = 10,191: as wide as the notebook's own float32 gradients
are, and wide enough that one row in 32,801 may go missing unseen.  The kernel's
header promises more: a row with a zero head gradient contributes an exact zero
to every gradient.  On rows that are dead in that sense (np.resize of the
fixture states, so not zeros: a dead row's state must not leak either) a few
live rows are placed, "content j" being fixture row j of states with its
float32 head-gradient row, and the result is compared with the calls at m = 1
on those contents alone.  BL = 256 blocks (kGradBlocks), TR = 128 rows a tile
(kTileRows), u = 2^-24; "equal" is np.array_equal on float32 (-0 == +0).  Both
networks (actor K = 3, critic K = 1) in every test.

1. One live row gives the same bits wherever it sits (m = 2 BL TR + 33 =
   65,569: block 0 takes a third, ragged tile; POSITIONS: the edges of every
   32-row wave, the first and last block, the second tile of a block, the
   ragged tile and its last row).  All fourteen gradients equal the m = 1
   call's and grad_norm has the same bits.  Exact because every other
   contribution is an exact zero, fma(0, a, acc) = acc, the per-row arithmetic
   does not depend on the lane, the double sum over blocks of one value and 255
   zeros is that value, and the norm's tree adds the same values.
2. The partials are added in block order, in double, rounded once (m = 2 BL
   TR).  Block b has one live row, in tile b (b even) or b + 256 (b odd), at
   (37 b) mod 128 in the tile, of content b mod 16, so by 1 its partial is the
   single-row result g_(b mod 16) and every element equals float32(sum over b =
   0..255, in that order, of float64(g_(b mod 16))).  grad_norm within 1e-11
   relative of sqrt(sum float64(f)^2) over the returned gradients: the kernel's
   tree and NumPy add at most 27,651 doubles in different orders, 27,651 x
   2^-53 = 3.1e-12.
3. Two live rows inside one block add up (m = 2 BL TR; PAIRS).  With g1, g2
   the single-row results, |got - (g1 + g2)| <= 2 u (|g1| + |g2|) + 2^-149: an
   accumulator or fmaf column sum holds round(g1 + p2), p2 the second row's
   unrounded product and g2 = round(p2), which costs u |g2| + u |g1 + p2|; a
   plain add is round(g1 + g2); a two-term MFMA step with one rounding is
   tighter.  Where g1 = g2 = 0 the result is 0.  Measured largest ratio to the
   bound: 0.93 on the MFMA-accumulated 0.weight, 3.weight, 6.weight (critic
   0.weight; 0.78 for the actor), 0.38 - 0.51 on every other tensor (a plain
   add's u |g1 + g2| is 0.5 of the bound): all fourteen tensors hold at 2.
4. The ReLU edge and dead LayerNorm units (mlp_backward_ref.crafted, derived
   from the fixture networks at run time).  "relu": gamma = 0 makes y = beta
   exactly, in float32 and float64 alike; units 3, 40, n - 1 of every LayerNorm
   have y = 0, -2^-100, 0 and pass nothing, units 17 and 0 have y = 2^-100 and
   pass every row's gradient, so [y > 0] and [y >= 0] differ on every row.
   "var0": 0.weight = 0, 0.bias = 0.25, so layer 1 has zero variance, xh = 0
   and rstd = 1 / sqrt(eps).  On the 203 fixture rows and on 1 row, against the
   restatement on the crafted weights under the neighbour's rule err <= 4 G u S
   with the fixture's G (tests/test_mlp_backward_cpu.py: float32 autograd's own
   gap there is 5,887 / 31 for the actor, 229 / 84 for the critic).  S = 0
   forces exact zeros, asserted by name too (mlp_backward_ref.crafted_zeros):
   dgamma and dbeta of the off units, the next Linear's dW column of every unit
   whose activation is 0; dbeta_17 is nonzero wherever the restatement's is.
"""
import numpy as np
import pytest
import torch

import mlp_backward_ref as ref
from delivery_drone_amd import MlpNet
from delivery_drone_amd.policy import STATE_DICT_KEYS
from test_gpu_mlp_backward import (BLOCKS as BL, TILE_ROWS as TR, U, check_exact, fx, g, host, nets,  # noqa: F401
                                   reference)  # fx, g, nets, reference are fixtures

pytestmark = pytest.mark.gpu

TAGS = ("actor", "critic")
M_BIG = 2 * BL * TR + 33
POSITIONS = (0, 1, 31, 32, 33, 63, 64, 96, 127, 128, 129, 32767, 32768, 32895, 32966, 65535, 65536, 65568)
# (rows, contents): the contents differ within a pair and are among part 1's, whose m = 1 results are shared
PAIRS = (((6, 7), (0, 17)),               # the same k-step of the dW MFMA
         ((3, 20), (1, 16)),              # the same wave
         ((5, 100), (2, 15)),             # two waves of one tile
         ((10, 70), (3, 14)),             # two row quarters and two row halves of the column sums
         ((9, 32768 + 9), (4, 13)),       # one block, two tiles, the same lane
         ((9, 32768 + 77), (5, 12)))      # one block, two tiles, another wave


class Bench:
    """One network on the device with the dead background (built once) and the
    fixture contents; live rows are patched in on the device and taken out
    again after the call."""

    def __init__(self, tag, sd, states, head, dev):
        self.tag, self.net, self.dev = tag, MlpNet(sd, device=dev), dev
        self.rows = torch.as_tensor(np.ascontiguousarray(states), device=dev)
        self.head = torch.as_tensor(np.ascontiguousarray(head), device=dev)
        self.bg = torch.as_tensor(np.resize(states, (M_BIG, 15)), device=dev)
        self.states = self.bg.clone()
        self.grad_out = torch.zeros((M_BIG,) + tuple(head.shape[1:]), dtype=torch.float32, device=dev)
        self._single = {}

    def single(self, j):
        """(gradients on the host, grad_norm on the device) of content j at m = 1."""
        if j not in self._single:
            assert bool(self.head[j].ne(0).any()), f"content {j} has a zero head gradient"
            grads, norm = self.net.backward(self.rows[j:j + 1], self.head[j:j + 1])
            out = {k: host(grads[k]).copy() for k in STATE_DICT_KEYS}
            assert np.any(out["9.bias"] != 0) and np.any(out["0.weight"] != 0), j
            self._single[j] = (out, norm)
        return self._single[j]

    def placed(self, m, live):
        """The call on the first m background rows with content j at row pos
        for every (pos, j) of live."""
        pos = torch.as_tensor([p for p, _ in live], device=self.dev)
        src = torch.as_tensor([j for _, j in live], device=self.dev)
        assert len(set(p for p, _ in live)) == len(live) and max(p for p, _ in live) < m <= M_BIG
        self.states[pos] = self.rows[src]
        self.grad_out[pos] = self.head[src]
        grads, norm = self.net.backward(self.states[:m], self.grad_out[:m])
        out = {k: host(grads[k]).copy() for k in STATE_DICT_KEYS}
        self.states[pos] = self.bg[pos]
        self.grad_out[pos] = 0.0
        return out, norm


@pytest.fixture(scope="module")
def benches(g, nets, reference, gpu_device):  # noqa: F811
    return {tag: Bench(tag, nets[tag], g["states"], reference["head"][tag], gpu_device) for tag in TAGS}


# ---- 1 ---------------------------------------------------------------------------------

@pytest.mark.parametrize("tag", TAGS)
def test_a_live_row_gives_the_same_bits_wherever_it_sits(benches, tag):
    b = benches[tag]
    bad = []
    for i, pos in enumerate(POSITIONS):
        j = i % len(b.rows)
        want, want_norm = b.single(j)
        got, norm = b.placed(M_BIG, [(pos, j)])
        for k in STATE_DICT_KEYS:
            if not np.array_equal(got[k], want[k]):
                n = int((got[k] != want[k]).sum())
                bad.append(f"row {pos} (block {pos // TR % BL}, tile {pos // TR}, in-tile {pos % TR}) {k}: "
                           f"{n} of {got[k].size} elements differ, largest {np.abs(got[k] - want[k]).max():.3g}")
        if not torch.equal(norm, want_norm):
            bad.append(f"row {pos} grad_norm {float(norm)!r} != {float(want_norm)!r}")
    assert not bad, "\n".join(bad)


# ---- 2 ---------------------------------------------------------------------------------

@pytest.mark.parametrize("tag", TAGS)
def test_partials_are_added_in_block_order_in_double(benches, tag):
    b = benches[tag]
    live = []
    for blk in range(BL):
        tile = blk if blk % 2 == 0 else blk + BL
        live.append((tile * TR + (37 * blk) % TR, blk % 16))
    assert all(pos // TR % BL == blk for blk, (pos, _) in enumerate(live))
    got, norm = b.placed(2 * BL * TR, live)
    sq = 0.0
    for k in STATE_DICT_KEYS:
        s = np.zeros(got[k].shape, np.float64)
        for blk in range(BL):  # in block order
            s = s + b.single(blk % 16)[0][k].astype(np.float64)
        want = s.astype(np.float32)
        assert np.array_equal(got[k], want), \
            (f"{k}: {int((got[k] != want).sum())} of {want.size} elements differ, "
             f"largest {np.abs(got[k] - want).max():.3g}")
        sq += float((got[k].astype(np.float64) ** 2).sum())
    print(f"{tag} grad_norm {float(norm)!r} want {np.sqrt(sq)!r}")
    assert abs(float(norm) - np.sqrt(sq)) <= 1e-11 * np.sqrt(sq)


# ---- 3 ---------------------------------------------------------------------------------

@pytest.mark.parametrize("tag", TAGS)
def test_two_live_rows_of_one_block_add_up(benches, tag):
    b = benches[tag]
    worst, bad = {k: 0.0 for k in STATE_DICT_KEYS}, []
    for (r1, r2), (j1, j2) in PAIRS:
        assert r1 // TR % BL == r2 // TR % BL and j1 != j2
        g1, g2 = b.single(j1)[0], b.single(j2)[0]
        got, _ = b.placed(2 * BL * TR, [(r1, j1), (r2, j2)])
        for k in STATE_DICT_KEYS:
            a1, a2 = g1[k].astype(np.float64), g2[k].astype(np.float64)
            err = np.abs(got[k].astype(np.float64) - (a1 + a2))
            bound = 2.0 * U * (np.abs(a1) + np.abs(a2)) + 2.0 ** -149
            ratio = float((err / bound).max())
            worst[k] = max(worst[k], ratio)
            if ratio > 1.0:
                bad.append(f"rows ({r1}, {r2}) {k}: {int((err > bound).sum())} elements above the bound, "
                           f"ratio {ratio:.3g}")
            both = (g1[k] == 0) & (g2[k] == 0)
            if np.any(got[k][both] != 0):
                bad.append(f"rows ({r1}, {r2}) {k}: nonzero where both single-row results are zero")
    for k in STATE_DICT_KEYS:
        print(f"{tag} {k}: largest |got - (g1 + g2)| / bound {worst[k]:.3g}")
    assert not bad, "\n".join(bad)


# ---- 4 ---------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [203, 1])
@pytest.mark.parametrize("variant", ref.VARIANTS)
@pytest.mark.parametrize("tag", TAGS)
def test_relu_edge_and_dead_layernorm_units(g, nets, reference, gpu_device, tag, variant, n):  # noqa: F811
    sd = ref.crafted(nets[tag], variant)
    net = MlpNet(sd, device=gpu_device)
    states, head = g["states"][:n], reference["head"][tag][:n]
    grads, norm = net.backward(torch.as_tensor(states, device=gpu_device), torch.as_tensor(head, device=gpu_device))
    want, S, _ = check_exact(grads, norm, sd, states, head, reference["G"], f"{tag} {variant} n={n}")
    got = {k: host(grads[k]) for k in STATE_DICT_KEYS}
    for name, (k, idx) in ref.crafted_zeros(sd, variant).items():
        assert not np.any(S[k][idx]), name  # the restatement agrees that it is a forced zero
        assert not np.any(got[k][idx]), f"{name}: {got[k][idx]!r}"
    if variant == "relu":
        for _, ln in ref.LAYERS:
            for j in ref.RELU_ON:  # y = 2^-100 > 0: the gradient passes
                w = want[ln + ".bias"][j]
                assert w == 0 or got[ln + ".bias"][j] != 0, f"dbeta {ln}.bias[{j}] is zero, the restatement's {w!r}"
