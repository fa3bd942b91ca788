"""CPU record (oracle ops, fp64 algebra) for the FRePo trainer that is to come: how far the kernel ridge predictor moves when the
FEATURES it is given carry the relative rounding of the embedding passes -- 2^-11 (single-pass f16 operands) or 2^-22 (hi+lo
pairs).  The system's condition number multiplies feature error, so this prices which operand precision such a trainer may use.

Network: the oracle's ConvNet3D (oracle/ref_cpu.py) at 64x64x8, seed 1234; 6 synthetic and 8 target clips of randn pixels, C = 3,
reg 1e-6, the reference's loss line on one-hot targets.  A perturbed feature is f (1 + e u), u uniform in [-1, 1] per element,
applied to the synthetic and the target features alike.  Cases: independent clips, and two near-duplicate synthetic clips (clip 1
= clip 0 + 1e-3 randn, clip 3 = clip 2 + 1e-3 randn: what distillation drives same-class memories towards).  Reported per case and
e: cond_2(A), and the rel-L2 distance of pred, the relative distance of the loss and the rel-L2 distance of d loss / d feat_syn
from the unperturbed fp64 values (median of 5 draws of u).  No thresholds: a record; its output is the table of DESIGN.md
section 19.  Lives with the tests' tools: it imports the oracle.  Not collected by pytest."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import ref_cpu as R
from tests import nfr_oracle as O

torch.set_num_threads(8)


def loss_and_gradient(fs, ys, ft, y_tar, reg):
    fs = fs.double().clone().requires_grad_(True)
    kss, kts = fs @ fs.t(), ft.double() @ fs.t()
    n = kss.shape[0]
    pred = kts @ torch.linalg.solve(kss + abs(reg) * torch.trace(kss) * torch.eye(n, dtype=torch.float64) / n, ys.double())
    loss = torch.nn.functional.mse_loss(pred, y_tar.double(), reduction='none').sum(-1).mean(0)
    (g,) = torch.autograd.grad(loss, fs)
    return pred.detach(), float(loss.detach()), g


def main():
    n, m, C, reg = 6, 8, 3, 1e-6
    params = R.init_params(1234)
    print("%-16s %-6s %10s %12s %12s %12s" % ("case", "e", "cond_2(A)", "pred", "loss", "g_feat_syn"))
    for name in ("independent", "near-duplicates"):
        g = torch.Generator().manual_seed(19)
        x_syn = torch.randn(n, 8, 3, 64, 64, generator=g)
        x_tar = torch.randn(m, 8, 3, 64, 64, generator=g)
        if name == "near-duplicates":
            x_syn[1] = x_syn[0] + 1e-3 * torch.randn(8, 3, 64, 64, generator=g)
            x_syn[3] = x_syn[2] + 1e-3 * torch.randn(8, 3, 64, 64, generator=g)
        with torch.no_grad():
            fs, ft = R.convnet3d_embed(x_syn, params), R.convnet3d_embed(x_tar, params)
        ys = torch.nn.functional.one_hot(torch.arange(n) % C, C).float() - 1.0 / C
        y_tar = torch.nn.functional.one_hot(torch.arange(m) % C, C).float()
        pred0, loss0, g0 = loss_and_gradient(fs, ys, ft, y_tar, reg)
        cond = O.cond(fs, reg)
        for label, e in (("2^-11", 2.0 ** -11), ("2^-22", 2.0 ** -22)):
            rows = []
            for draw in range(5):
                gu = torch.Generator().manual_seed(100 + draw)
                ps = fs.double() * (1 + e * (2 * torch.rand(fs.shape, generator=gu, dtype=torch.float64) - 1))
                pt = ft.double() * (1 + e * (2 * torch.rand(ft.shape, generator=gu, dtype=torch.float64) - 1))
                pred, loss, gr = loss_and_gradient(ps, ys, pt, y_tar, reg)
                rows.append((O.rel_l2(pred, pred0), abs(loss - loss0) / abs(loss0), O.rel_l2(gr, g0)))
            med = np.median(np.array(rows), axis=0)
            print("%-16s %-6s %10.3e %12.2e %12.2e %12.2e" % (name, label, cond, med[0], med[1], med[2]))


if __name__ == "__main__":
    main()
