"""The constants of pointwise_checks.py against its CPU emulation of the instance norm and the streaming helpers of
csrc/pointwise.hip, and the conditioning of the one-pass row sums as a stated property.  No kernel launches here."""
import torch

import pointwise_checks as pc


def test_emulation_stays_within_half_of_each_constant():
    worst = pc.emulation_worst()
    print("[pointwise] emulation worst ratios: " + ", ".join(f"{k} {v:.2f}" for k, v in worst.items()))
    assert set(worst) == set(pc.C) == set(pc.EMU_WORST)
    for k, v in worst.items():
        assert v <= pc.C[k] / 2, (k, v, pc.C[k])
        assert v <= pc.EMU_WORST[k] * 1.02 + 0.01, f"{k}: the emulation reaches {v:.3f}, the module records {pc.EMU_WORST[k]}"


def test_the_rstd_of_one_pass_sums_is_conditioned_by_mean_over_std_squared():
    """In its own (one-pass) unit the emulation stays within half of the constant at every mean / std; in the two-pass unit of
    toknorm_checks.py it is more than 20 times out at N(50, 1): the cost of ``E[x^2] - mean^2`` on fp32 partial sums, pinned."""
    table = pc.conditioning_table()
    for dist, (rel, two, one) in table.items():
        print(f"[pointwise] {dist}: rstd relative error {rel:.2e}, {two:.1f} two-pass units, {one:.2f} one-pass units")
        assert one <= pc.C["rstd"] / 2, (dist, one)
        assert rel <= pc.EMU_TABLE[dist][0] * 1.05 and two <= pc.EMU_TABLE[dist][1] * 1.05 and one <= pc.EMU_TABLE[dist][2] * 1.05, dist
    assert table["n53"][1] <= 4 and table["n53"][0] <= 1e-6                # nothing to see at N(5, 3^2) ...
    assert table["n501"][1] > 20 and table["n5001"][1] > 200               # ... (mean / std)^2 later
    assert table["n501"][0] > 100 * table["n53"][0]


def test_a_defect_is_far_outside_the_bounds():
    """A workgroup's partial sums lost (the second chunk of a row) and a row that takes its neighbour's parameters."""
    t = pc.make_inputs(6, 16392, 3, "n53", 0)
    ref = pc.instnorm_reference(t["x"], t["w"], t["b"], 3, pc.EPS, t["gy"])
    x = t["x"].clone()
    x[:, pc.CHUNK:2 * pc.CHUNK] = 0.0                                      # what the sums see
    bad = pc.emulate_instnorm(x, t["w"], t["b"], 3)["stats"]
    assert float(pc.excess_ratio(bad[:, 0], ref["mean"], ref["unit_mean"]).max()) > 20 * pc.C["mean"]
    assert float(pc.excess_ratio(bad[:, 1], ref["rstd"], ref["unit_rstd"]).max()) > 20 * pc.C["rstd"]
    emu = pc.emulate_instnorm(t["x"], t["w"].roll(1), t["b"].roll(1), 3, pc.EPS, t["gy"])
    assert float(pc.excess_ratio(emu["y"], ref["y"], ref["unit_y"]).max()) > 20 * pc.C["y"]
    assert float(pc.excess_ratio(emu["gx"], ref["gx"], ref["unit_gx"]).max()) > 20 * pc.C["gx"]


def test_row_sums_are_the_plain_sums():
    x = torch.randn(3, 8200)
    assert torch.allclose(pc.row_sums(x), x.double().sum(1), rtol=0, atol=1e-3)
    assert torch.allclose(pc.row_sums(x, x), x.double().square().sum(1), rtol=1e-6)
