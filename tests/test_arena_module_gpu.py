"""etpnav_amd.arena.FrozenArenaModule on an MI355X, through its three subclasses at their smallest configurations (bf16 mode: every one
of them then forwards from an operand copy of its matrices, a bf16 shadow or depth's packed weights).

  move     a module built on the CPU, loaded and moved with .to("cuda") gives the bits of one built on the device with the same weights
  versions an in-place edit of one matrix through its nn.Parameter changes the next forward, for the moved module (whose parameters were
           re-pointed with `.data =` and keep their OWN version counters, which the arena's counter no longer sees) as for the
           device-built one (whose parameters share the arena's counter); restoring the value restores the first output's bits
"""
import pytest
import torch

from etpnav_amd.clip import CLIPEncoder
from etpnav_amd.depth import DepthEncoder
from etpnav_amd.waypoint import BinaryDistPredictorTRM

pytestmark = pytest.mark.gpu


def _clip(device):
    return CLIPEncoder(device=device, dtype=torch.bfloat16, image_size=32, layers=1)


def _depth(device):
    return DepthEncoder(device=device, dtype=torch.bfloat16, image_size=64, base_planes=16, blocks=(1, 1, 1, 1))


def _waypoint(device):
    return BinaryDistPredictorTRM(device=device, dtype=torch.bfloat16)


def _inputs(kind, g):
    if kind == "clip":
        return {"rgb": torch.randint(0, 256, (1, 32, 32, 3), generator=g, dtype=torch.uint8).cuda()}
    if kind == "depth":
        return {"depth": torch.rand(1, 64, 64, 1, generator=g).cuda()}
    return torch.randn(12, 2048, generator=g).cuda()


def _run(kind, mod, x):
    y = mod(None, x) if kind == "waypoint" else mod(x)
    torch.cuda.synchronize()
    return y.clone()


def _weights(mod, g):
    """norm scales near 1, every other vector and every matrix small and random: finite activations, no symmetric cancellations"""
    W = {}
    for name, shape, _ in mod.table:
        t = torch.randn(shape, generator=g)
        W[name] = 1.0 + 0.1 * t if (len(shape) == 1 and name.endswith("weight")) else 0.05 * t
    return W


CASES = {"clip": (_clip, "proj"), "depth": (_depth, "compression.0.weight"), "waypoint": (_waypoint, "vis_classifier.0.weight")}


@pytest.mark.parametrize("kind", sorted(CASES))
def test_moved_module_equals_device_built_and_both_see_parameter_edits(kind):
    make, edited = CASES[kind]
    g = torch.Generator().manual_seed(11)
    moved = make("cpu")
    W = _weights(moved, g)
    moved.load_state_dict(W, strict=True)
    assert moved.arena.device.type == "cpu"
    moved.to("cuda")
    built = make("cuda")
    built.load_state_dict(W, strict=True)
    x = _inputs(kind, g)
    y0 = _run(kind, built, x)
    assert torch.isfinite(y0).all() and float(y0.abs().max()) > 0
    assert torch.equal(_run(kind, moved, x), y0)
    for mod in (moved, built):
        p = dict(mod.named_parameters())[edited]
        offset = {n: off for n, _, off in mod.table}[edited]
        assert offset < mod.n_matrix and p.data_ptr() == mod.arena.data_ptr() + 4 * offset      # a matrix, and a view of the bound arena
        saved = p.detach().clone()
        with torch.no_grad():
            p.add_(0.05 * torch.randn(p.shape, generator=g).cuda())
        assert not torch.equal(_run(kind, mod, x), y0), "the operand copy was not rebuilt after an in-place parameter edit"
        with torch.no_grad():
            p.copy_(saved)
        assert torch.equal(_run(kind, mod, x), y0)
