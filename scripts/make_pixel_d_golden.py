"""Writes tests/golden/f11_pixel_d.npz: the state_dict of the reference's pixel discriminator under torch.manual_seed(0) and its fp32
output on one seeded 2 x 4 x 8 x 8 input.

    python scripts/make_pixel_d_golden.py <checkout of the reference project>

The reference's model/networks.py is IMPORTED from that checkout (``define_D(4, 64, 'pixel', norm='instance', init_type='normal',
init_gain=0.02)``); nothing of it is restated here.  With ``--stock`` the same fixture is built from stock torch.nn with the same seed
(Conv2d / InstanceNorm2d constructors in the same order, N(0, 0.02) weights, zero biases) for a machine where the reference does not
import.  Only the output is committed; the tests read the fixture, never the reference.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "f11_pixel_d.npz")


def reference_net(path):
    sys.path.insert(0, path)
    from model import networks                      # the reference's module, from its checkout
    torch.manual_seed(0)
    return networks.define_D(4, 64, "pixel", norm="instance", init_type="normal", init_gain=0.02)


def stock_net():
    nn = torch.nn
    torch.manual_seed(0)

    class Net(nn.Module):
        def __init__(self):
            super().__init__()
            self.net = nn.Sequential(nn.Conv2d(4, 64, 1), nn.LeakyReLU(0.2, True), nn.Conv2d(64, 128, 1), nn.InstanceNorm2d(128),
                                     nn.LeakyReLU(0.2, True), nn.Conv2d(128, 1, 1))

        def forward(self, x):
            return self.net(x)
    net = Net()
    for m in net.net:
        if isinstance(m, nn.Conv2d):
            nn.init.normal_(m.weight.data, 0.0, 0.02)
            nn.init.constant_(m.bias.data, 0.0)
    return net


def main(argv):
    if len(argv) != 2:
        raise SystemExit(__doc__)
    net = stock_net() if argv[1] == "--stock" else reference_net(argv[1])
    net = net.float().cpu().eval()
    x = torch.rand(2, 4, 8, 8, generator=torch.Generator().manual_seed(1)) * 2 - 1
    with torch.no_grad():
        out = net(x)
    arrays = {"sd/" + k: v.detach().numpy() for k, v in net.state_dict().items()}
    arrays["x"], arrays["out"] = x.numpy(), out.numpy()
    arrays["source"] = np.array("stock torch.nn" if argv[1] == "--stock" else "reference define_D")
    np.savez(OUT, **arrays)
    print("wrote", OUT, {k: v.shape for k, v in arrays.items()})


if __name__ == "__main__":
    main(sys.argv)
