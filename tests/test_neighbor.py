"""CPU tests of the Neighbor2Neighbor pairs (blind_image_denoising_amd/neighbor.py): the properties of the NumPy restatement in
tests/neighbor_reference.py -- the yardstick of the GPU tests -- the identity that folds the paper's regulariser into the target,
the argument checks that fire before a device is touched, and the `train.self_supervised` parser."""
import numpy as np
import pytest
import torch

import blind_image_denoising_amd as bf
from blind_image_denoising_amd import neighbor as NB
import neighbor_reference as R

SEEDS = (0, 2 ** 40 + 12345, 2 ** 64 - 1, 7)
B, H, W, C = 3, 64, 96, 3


# ---- the reference ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", SEEDS)
def test_reference_pairs_are_adjacent_pixels_of_the_cell(seed):
    k = R.choices(B, H, W, seed)
    assert k.shape == (B, H // 2, W // 2) and k.min() >= 0 and k.max() <= 7
    p1, p2 = R.positions(k)
    assert (p1 != p2).all()
    # 4-adjacent, never diagonal: exactly one of (row, column) differs
    assert (((p1 >> 1) != (p2 >> 1)).astype(int) + ((p1 & 1) != (p2 & 1)).astype(int) == 1).all()
    # both come from the cell: an image that holds its own cell number gives that number back in both outputs
    cell = np.arange((H // 2) * (W // 2), dtype=np.float32).reshape(H // 2, W // 2)
    y = np.broadcast_to(np.kron(cell, np.ones((2, 2), np.float32))[None, :, :, None], (B, H, W, C)).copy()
    inp, tgt = R.pairs(y, seed)
    assert (inp == cell[None, :, :, None]).all() and (tgt == cell[None, :, :, None]).all()
    # and from the drawn position: an image that holds the position number gives (p1, p2) back, the same for every channel
    pos = np.broadcast_to(np.tile(np.array([[0, 1], [2, 3]], np.uint8), (H // 2, W // 2))[None, :, :, None], (B, H, W, C)).copy()
    inp, tgt = R.pairs(pos, seed)
    assert (inp == p1[..., None]).all() and (tgt == p2[..., None]).all() and inp.dtype == np.float32


@pytest.mark.parametrize("seed", SEEDS)
def test_reference_draws_every_pair_uniformly(seed):
    """every k occurs, each within 5 binomial standard deviations of 1/8 over the 3 * 32 * 48 cells"""
    k = R.choices(B, H, W, seed)
    n = k.size
    counts = np.bincount(k.reshape(-1), minlength=8)
    sd = np.sqrt(n * (1 / 8) * (7 / 8))
    assert (counts > 0).all() and (np.abs(counts - n / 8) <= 5 * sd).all(), counts


def test_reference_draws_differ_per_image_and_seed_and_repeat():
    k = R.choices(B, H, W, 5)
    assert (k[0] != k[1]).any() and (k[1] != k[2]).any()
    assert (k != R.choices(B, H, W, 6)).any()
    assert (k == R.choices(B, H, W, 5)).all()
    assert (k[:2] == R.choices(2, H, W, 5)).all()                    # an image's draw does not depend on the batch size


def test_reference_groups_do_not_straddle_rows():
    """W2 = 5: two groups per row, the second one cell wide; the first cell of every row starts a group (word 0)"""
    k = R.choices(1, 6, 10, 3)
    g = np.arange(3, dtype=np.uint64) * np.uint64(2)
    words = R.O._philox4x32_10(g, np.zeros_like(g), np.zeros_like(g), np.full_like(g, 3), 3, 0)
    assert (k[0, :, 0] == (words[0] >> np.uint64(29)).astype(np.int64)).all()
    words = R.O._philox4x32_10(g + np.uint64(1), np.zeros_like(g), np.zeros_like(g), np.full_like(g, 3), 3, 0)
    assert (k[0, :, 4] == (words[0] >> np.uint64(29)).astype(np.int64)).all()


def test_reference_target_blends_the_difference_of_the_denoised_pair():
    rng = np.random.default_rng(0)
    y = rng.integers(0, 256, (2, 8, 12, 3), dtype=np.uint8)
    f = rng.uniform(0, 255, y.shape).astype(np.float32)
    inp, tgt = R.pairs(y, 11, f, 0.25)
    g1, g2 = R.pairs(f, 11)
    y1, y2 = R.pairs(y, 11)
    assert (inp == y1).all() and tgt.dtype == np.float64
    assert np.array_equal(tgt, y2.astype(np.float64) + 0.25 * (g1 - g2).astype(np.float64))


# ---- the target identity ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("gamma", [0.0, 0.5, 2.0, 8.0])
def test_folding_the_regulariser_into_the_target_keeps_the_gradient(gamma):
    """d/dp [ |p - g2|^2 + gamma |p - g2 - d|^2 ] = (1 + gamma) d/dp |p - (g2 + gamma / (1 + gamma) d)|^2, in fp64 autograd"""
    gen = torch.Generator().manual_seed(int(gamma * 10))
    p, g2, d = (torch.randn(2, 6, 8, 3, dtype=torch.float64, generator=gen) * s for s in (30.0, 30.0, 5.0))
    p.requires_grad_(True)
    paper = ((p - g2) ** 2).sum() + gamma * ((p - g2 - d) ** 2).sum()
    grad_paper, = torch.autograd.grad(paper, p)
    folded = ((p - (g2 + gamma / (1.0 + gamma) * d)) ** 2).sum()
    grad_folded, = torch.autograd.grad(folded, p)
    err = (grad_paper - (1.0 + gamma) * grad_folded).abs().max().item()
    assert err <= 1e-12 * grad_paper.abs().max().item(), err
    # and the two losses differ by a constant in p
    q = torch.randn(p.shape, dtype=torch.float64, generator=gen)
    at = lambda v: (((v - g2) ** 2).sum() + gamma * ((v - g2 - d) ** 2).sum() - (1 + gamma) * ((v - (g2 + gamma / (1 + gamma) * d)) ** 2).sum()).item()
    assert abs(at(p.detach()) - at(q)) <= 1e-9 * abs(paper.item())


# ---- argument checks, before a device is touched ----------------------------------------------------------------------------------

_Y = torch.zeros((1, 8, 8, 3), dtype=torch.uint8)


@pytest.mark.parametrize("bad", [torch.zeros((8, 8, 3), dtype=torch.uint8), torch.zeros((1, 8, 8, 3), dtype=torch.float64),
                                 torch.zeros((1, 7, 8, 3)), torch.zeros((1, 8, 9, 3)), torch.zeros((1, 8, 8, 5)), torch.zeros((0, 8, 8, 3)),
                                 torch.zeros((1, 0, 8, 3)), np.zeros((1, 8, 8, 3), np.uint8), None], ids=lambda b: str(getattr(b, "shape", b)))
def test_neighbor_pairs_refuses_bad_batches_without_a_device(bad):
    with pytest.raises(ValueError):
        bf.neighbor_pairs(bad)


@pytest.mark.parametrize("kw", [{"weight": 1.0}, {"weight": -0.1}, {"weight": float("nan")}, {"weight": float("inf")}, {"weight": True},
                                {"weight": 1.0 - 1e-12}, {"seed": -1}, {"seed": 2 ** 64}, {"seed": 1.5},
                                {"denoised": torch.zeros((1, 8, 8, 3), dtype=torch.uint8)}, {"denoised": torch.zeros((1, 8, 6, 3))},
                                {"denoised": torch.zeros((2, 8, 8, 3))}, {"denoised": np.zeros((1, 8, 8, 3), np.float32)}], ids=str)
def test_neighbor_pairs_refuses_bad_arguments_without_a_device(kw):
    with pytest.raises(ValueError):
        bf.neighbor_pairs(_Y, **kw)


def test_neighbor_pairs_does_not_upload_host_tensors():
    with pytest.raises(RuntimeError, match="GPU"):
        bf.neighbor_pairs(_Y)
    with pytest.raises(RuntimeError, match="GPU"):
        bf.neighbor_pairs(_Y.float(), 3, torch.zeros((1, 8, 8, 3)), 0.5)


def test_neighbor_pairs_dataset_checks_its_arguments():
    for gamma in (-1.0, float("nan"), float("inf"), "2", True):
        with pytest.raises(ValueError, match="gamma"):
            bf.NeighborPairs([_Y], model=lambda u: u.float(), gamma=gamma)
    with pytest.raises(ValueError, match="model"):
        bf.NeighborPairs([_Y], gamma=1.0)
    with pytest.raises(ValueError, match="model"):
        bf.NeighborPairs([_Y], model=3, gamma=1.0)
    with pytest.raises(ValueError, match="batches"):
        bf.NeighborPairs(None)
    for bad in ([torch.zeros((1, 7, 8, 3))], [(_Y, _Y, _Y)], [(None, torch.zeros((8, 8, 3)))], [(None, "noisy")]):
        with pytest.raises(ValueError):
            next(iter(bf.NeighborPairs(bad)))


def test_neighbor_pairs_dataset_weight_follows_the_ramp():
    ds = bf.NeighborPairs([_Y], model=lambda u: u.float(), gamma=2.0, ramp=True)
    assert ds.percentage_done == 0.0 and ds.weight() == 0.0
    ds.percentage_done = 0.5
    assert ds.weight() == pytest.approx(0.5)                         # gamma_t = 1
    ds.percentage_done = 1.0
    assert ds.weight() == pytest.approx(2.0 / 3.0)
    assert bf.NeighborPairs([_Y], model=lambda u: u.float(), gamma=2.0, ramp=False).weight() == pytest.approx(2.0 / 3.0)
    assert bf.NeighborPairs([_Y]).weight() == 0.0


# ---- the train.self_supervised section ------------------------------------------------------------------------------------------------

def test_self_supervised_section_defaults_and_values():
    assert bf.parse_self_supervised_config({"epochs": 1}) is None
    c = bf.parse_self_supervised_config({"self_supervised": {"type": "neighbor2neighbor"}})
    assert c == NB.SelfSupervisedConfig("neighbor2neighbor", 0.0, True, None)
    c = bf.parse_self_supervised_config({"self_supervised": {"type": "Neighbor2Neighbor", "gamma": 2, "ramp": False, "validation": {}}})
    assert c.gamma == 2.0 and c.ramp is False
    assert c.validation == NB.RiskValidationConfig(every=0, inputs=[], sigma=None, method="mad", probes=1)
    v = bf.parse_self_supervised_config({"self_supervised": {"type": "neighbor2neighbor", "validation": {
        "every": 50, "inputs": "held", "sigma": 20, "method": "immerkaer", "probes": 2}}}).validation
    assert v == NB.RiskValidationConfig(every=50, inputs=["held"], sigma=20.0, method="immerkaer", probes=2)


@pytest.mark.parametrize("section", [{"type": "noise2void"}, {}, {"gamma": 1.0}, "neighbor2neighbor", {"type": "neighbor2neighbor", "gamma": -1},
                                     {"type": "neighbor2neighbor", "gamma": "2"}, {"type": "neighbor2neighbor", "ramp": 1},
                                     {"type": "neighbor2neighbor", "lambda": 0.5}, {"type": "neighbor2neighbor", "validation": {"each": 5}},
                                     {"type": "neighbor2neighbor", "validation": {"probes": 9}},
                                     {"type": "neighbor2neighbor", "validation": {"method": "median"}},
                                     {"type": "neighbor2neighbor", "validation": {"sigma": -1}}], ids=str)
def test_self_supervised_section_refuses_what_it_does_not_know(section):
    with pytest.raises(ValueError):
        bf.parse_self_supervised_config({"self_supervised": section})


def test_the_entry_point_is_bound():
    from blind_image_denoising_amd import _native as N
    assert "bf_op_neighbor_pairs" in N.SIGNATURES and hasattr(N.lib(), "bf_op_neighbor_pairs")
