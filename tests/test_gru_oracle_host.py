"""The GRU references the GPU tests are judged by (oracle.pmce_oracle.gru_step / gru_bidir2) against torch.nn.GRU / nn.GRUCell in fp64 on the
same weights, on the host: a reference that shared a kernel's mistake (gate order, which bias the reset gate multiplies, the direction
of the backward walk, what layer 1 reads) would fail here.  Agreement is at fp64 rounding: 1e-12 on values of order 1."""
import torch

from oracle import pmce_oracle as O

TOL = 1e-12


def _gru(I, H, seed):
    torch.manual_seed(seed)
    gru = torch.nn.GRU(I, H, num_layers=2, bidirectional=True).double()
    with torch.no_grad():
        for p in gru.parameters():           # nn.GRU's own init is U(-1/sqrt(H), 1/sqrt(H)): widen it so the gates leave their linear range
            p.mul_(3.0)
    return gru


def test_gru_step_is_nn_grucell_fp64():
    I, H, B = 24, 16, 5
    gru = _gru(I, H, 3)
    sd = gru.state_dict()
    cell = torch.nn.GRUCell(I, H).double()
    g = torch.Generator().manual_seed(4)
    x = torch.randn(B, I, generator=g, dtype=torch.float64)
    h = torch.tanh(torch.randn(B, H, generator=g, dtype=torch.float64))
    for sfx in ("", "_reverse"):
        cell.load_state_dict({k: sd[f"{k}_l0{sfx}"] for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")})
        gi = torch.nn.functional.linear(x, sd[f"weight_ih_l0{sfx}"], sd[f"bias_ih_l0{sfx}"])
        with torch.no_grad():
            for hp, hp_ref in ((h, h), (None, torch.zeros(B, H, dtype=torch.float64))):
                got = O.gru_step(gi, sd[f"weight_hh_l0{sfx}"], sd[f"bias_hh_l0{sfx}"], hp)
                ref = cell(x, hp_ref)
                assert got.dtype == torch.float64 and float((got - ref).abs().max()) < TOL
        # fp32 inputs are widened, not computed in fp32
        got32 = O.gru_step(gi.float(), sd[f"weight_hh_l0{sfx}"].float(), sd[f"bias_hh_l0{sfx}"].float(), h.float())
        assert got32.dtype == torch.float64


def test_gru_bidir2_is_nn_gru_fp64_both_layers():
    I, H, B, Tn = 24, 16, 3, 7
    gru = _gru(I, H, 5)
    sd = {"gru." + k: v for k, v in gru.state_dict().items()}
    x = torch.randn(Tn, B, I, generator=torch.Generator().manual_seed(6), dtype=torch.float64)
    with torch.no_grad():
        ref_top, _ = gru(x)
        layer0 = torch.nn.GRU(I, H, num_layers=1, bidirectional=True).double()
        layer0.load_state_dict({k: v for k, v in gru.state_dict().items() if "_l0" in k})
        ref_l0, _ = layer0(x)
        top, l0 = O.gru_bidir2(x, sd, "gru", torch.float64, return_layer0=True)
        only_top = O.gru_bidir2(x, sd, "gru", torch.float64)
    assert top.shape == (Tn, B, 2 * H) and l0.shape == (Tn, B, 2 * H)
    e_top, e_l0 = float((top - ref_top).abs().max()), float((l0 - ref_l0).abs().max())
    print(f"gru_bidir2 fp64 vs nn.GRU fp64: top layer {e_top:.1e}, layer 0 {e_l0:.1e}; |y| up to {float(ref_top.abs().max()):.2f}")
    assert e_top < TOL and e_l0 < TOL
    assert torch.equal(only_top, top)
    assert float(ref_top.abs().max()) > 0.5          # values of order 1: the bound means something
    # the two directions really walk in opposite orders: the forward half at t = 0 and the backward half at t = T - 1 are first steps
    first_f = O.gru_step(torch.nn.functional.linear(x[0], sd["gru.weight_ih_l0"], sd["gru.bias_ih_l0"]), sd["gru.weight_hh_l0"], sd["gru.bias_hh_l0"])
    first_b = O.gru_step(torch.nn.functional.linear(x[-1], sd["gru.weight_ih_l0_reverse"], sd["gru.bias_ih_l0_reverse"]),
                         sd["gru.weight_hh_l0_reverse"], sd["gru.bias_hh_l0_reverse"])
    assert float((l0[0, :, :H] - first_f).abs().max()) < TOL and float((l0[-1, :, H:] - first_b).abs().max()) < TOL
