"""Model-level parity on the MI355X: the cfg-driven Darknet on HIP kernels vs (a) golden vectors minted
from the reference, (b) the CPU oracle on fresh seeded inputs.  Tolerance 1e-3 (north_star), fp32."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOL = 1e-3


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _mini(dev):
    from fewshot_detection_amd.darknet_meta import Darknet
    net = Darknet(os.path.join(GOLD, "mini_dynamic.cfg"), os.path.join(GOLD, "mini_reweight.cfg"))
    net.load_weights(os.path.join(GOLD, "mini.weights"))
    return net.to(dev)


def test_meta_detector_forward_vs_reference_golden(dev):
    d = np.load(os.path.join(GOLD, "mini_forward.npz"))
    net = _mini(dev)
    assert int(net.seen) == 4242
    x, metax, mask = (torch.from_numpy(d[k]).to(dev) for k in ("x", "metax", "mask"))
    net.eval()
    with torch.no_grad():
        dyn = net.meta_forward(metax, mask)
        out = net.detect_forward(x, dyn)
    assert dyn[0].shape == (3, 64, 1, 1) and out.shape == (6, 30, 2, 2)
    assert np.abs(dyn[0].cpu().numpy() - d["dyn_eval"]).max() < TOL
    assert np.abs(out.cpu().numpy() - d["out_eval"]).max() < TOL
    net.train()
    with torch.no_grad():
        out = net(x, metax, mask)
    assert np.abs(out.cpu().numpy() - d["out_train"]).max() < TOL
    sd = net.state_dict()
    assert np.allclose(sd["models.0.bn1.running_mean"].cpu().numpy(), d["bn1_mean_after"], atol=1e-5)
    assert np.allclose(sd["models.0.bn1.running_var"].cpu().numpy(), d["bn1_var_after"], atol=1e-5)
    assert np.allclose(sd["learnet_models.10.bn6.running_var"].cpu().numpy(), d["lbn6_var_after"], atol=1e-5)


def test_weights_roundtrip_byte_exact(dev, tmp_path):
    net = _mini(dev)
    p = str(tmp_path / "rt.weights")
    net.save_weights(p)
    assert open(p, "rb").read() == open(os.path.join(GOLD, "mini.weights"), "rb").read()


def test_plain_yolo_vs_reference_golden(dev):
    from fewshot_detection_amd.darknet import Darknet
    d = np.load(os.path.join(GOLD, "mini_yolo_forward.npz"))
    net = Darknet(os.path.join(GOLD, "mini_tiny_yolo.cfg"))
    net.load_weights(os.path.join(GOLD, "mini_yolo.weights"))
    net = net.to(dev)
    x = torch.from_numpy(d["x"]).to(dev)
    net.eval()
    with torch.no_grad():
        assert np.abs(net(x).cpu().numpy() - d["out_eval"]).max() < TOL
    net.train()
    with torch.no_grad():
        assert np.abs(net(x).cpu().numpy() - d["out_train"]).max() < TOL


@pytest.mark.parametrize("S,Sm,B,N", [(104, 104, 2, 3), (96, 64, 3, 2)])
def test_mini_detector_vs_oracle_odd_sizes(dev, S, Sm, B, N):
    """13x13 -> 6x6 floor pooling (S=104) and non-default support size, against the CPU oracle."""
    from fewshot_detection_amd.darknet_meta import Darknet
    from oracle.net import OracleDarknet
    torch.manual_seed(S)
    cfgs = (os.path.join(GOLD, "mini_dynamic.cfg"), os.path.join(GOLD, "mini_reweight.cfg"))
    ora = OracleDarknet(*cfgs)
    for m in ora.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.weight.data.uniform_(0.5, 1.5)
            m.bias.data.uniform_(-0.2, 0.2)
    net = Darknet(*cfgs)
    net.load_state_dict(ora.state_dict())
    net = net.to(dev)
    x, metax = torch.rand(B, 3, S, S), torch.rand(N, 3, Sm, Sm)
    mask = (torch.rand(N, 1, Sm, Sm) > 0.5).float()
    ora.train(); net.train()
    with torch.no_grad():
        ref = ora(x, metax, mask)
        out = net(x.to(dev), metax.to(dev), mask.to(dev))
    assert out.shape == ref.shape
    assert float((out.cpu() - ref).abs().max()) < TOL


def test_load_weights_after_a_forward_invalidates_packed_weights(dev, tmp_path):
    """eval.py:118-122 pushes several checkpoints through ONE model.  The packed / Winograd weight
    copies the engine caches must not survive load_weights (its `.data.copy_` leaves torch's version counter alone)."""
    from fewshot_detection_amd.darknet_meta import Darknet
    d = np.load(os.path.join(GOLD, "mini_forward.npz"))
    x, metax, mask = (torch.from_numpy(d[k]).to(dev) for k in ("x", "metax", "mask"))
    other = Darknet(os.path.join(GOLD, "mini_dynamic.cfg"), os.path.join(GOLD, "mini_reweight.cfg"))
    other.load_weights(os.path.join(GOLD, "mini.weights"))
    with torch.no_grad():                                       # a second checkpoint: every conv filter flipped and scaled
        for name, p in other.named_parameters():
            if "conv" in name and name.endswith("weight"):
                p.mul_(-0.7)
    p_other = str(tmp_path / "other.weights")
    other.save_weights(p_other)
    net = _mini(dev).eval()
    with torch.no_grad():
        first = net(x, metax, mask).clone()                     # fills the packed-weight cache
        net.load_weights(p_other)                               # second checkpoint through the same model
        second = net(x, metax, mask)
        fresh_net = Darknet(os.path.join(GOLD, "mini_dynamic.cfg"), os.path.join(GOLD, "mini_reweight.cfg"))
        fresh_net.load_weights(p_other)
        fresh = fresh_net.to(dev).eval()(x, metax, mask)
    assert float((first - second).abs().max()) > 1e-3          # the checkpoints really differ
    assert torch.equal(second, fresh)
    # a user's raw in-place edit through .data followed by the documented invalidation call
    from fewshot_detection_amd.engine import bump_weight_epoch
    with torch.no_grad():
        net.models[21][0].weight.data.mul_(-3.0)               # 96 -> 64 3x3: runs from the packed K-major copy
        bump_weight_epoch()
        third = net(x, metax, mask)
        fresh_net.models[21][0].weight.data.mul_(-3.0)
        bump_weight_epoch()
        fresh3 = fresh_net(x, metax, mask)
    assert float((third - second).abs().max()) > 1e-3 and torch.equal(third, fresh3)


def test_network_inputs_are_validated(dev):
    """wrong dtypes / mismatched mask sizes raise instead of being reinterpreted or scattered."""
    d = np.load(os.path.join(GOLD, "mini_forward.npz"))
    net = _mini(dev).eval()
    x, metax, mask = (torch.from_numpy(d[k]).to(dev) for k in ("x", "metax", "mask"))
    with torch.no_grad():
        with pytest.raises(ValueError):
            net(x.double(), metax, mask)
        with pytest.raises(ValueError):
            net(x, metax, (mask * 255).to(torch.uint8))
        with pytest.raises(ValueError):
            net(x, metax, torch.cat([mask, mask], 0))                      # more masks than supports
        with pytest.raises(ValueError):
            net(x, metax, mask[:, :, :mask.shape[2] // 2])                  # stale smaller mask
        dyn = net.meta_forward(metax, mask)
        with pytest.raises(ValueError):
            net.detect_forward(x, [dyn[0].half()])
        net.detect_forward(x, dyn)


def test_standalone_modules_are_shape_faithful(dev):
    """Reorg / MaxPool modules with C % 4 != 0 return the true channel count and ordering; a
    ConvBlock the HIP path cannot run says so."""
    import torch.nn as nn
    import torch.nn.functional as F
    from fewshot_detection_amd.darknet_meta import ConvBlock, MaxPool2x2, MaxPoolStride1, Reorg
    from oracle.net import reorg as oracle_reorg
    g = torch.Generator().manual_seed(3)
    for c in (3, 6, 8):
        x = torch.randn(2, c, 8, 6, generator=g)
        r = Reorg(2)(x.to(dev)).cpu()
        assert r.shape == (2, 4 * c, 4, 3) and torch.equal(r, oracle_reorg(x, 2))
        p = MaxPool2x2()(x.to(dev)).cpu()
        assert torch.equal(p, F.max_pool2d(x, 2, 2))
        p1 = MaxPoolStride1()(x.to(dev)).cpu()
        assert torch.equal(p1, F.max_pool2d(F.pad(x, (0, 1, 0, 1), mode="replicate"), 2, 1))
    blk = ConvBlock()
    blk.add_module("conv1", nn.Conv2d(4, 8, 3, 2, 1))
    with pytest.raises(NotImplementedError):
        blk.to(dev)(torch.randn(1, 4, 8, 8).to(dev))
    blk = ConvBlock()
    blk.add_module("conv1", nn.Conv2d(4, 8, 3, 1, 0))
    with pytest.raises(NotImplementedError):
        blk.to(dev)(torch.randn(1, 4, 8, 8).to(dev))


def test_bench_timed_region_allocates_no_device_memory():
    """VERDICT r5 #4 (bench smoke): the driver-shaped command on the headline episode, extras off -- after bench.py's settle phase
    (bursts of free-running steps, see Leg.run) the timed region must not call hipMalloc: every step of it reuses cached blocks."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "12", "--warmup", "3", "--no-extras",
           "--no-cpu-baseline", "--no-parity"]
    out = subprocess.run(cmd, cwd=root, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    d = json.loads(out.stdout.strip().splitlines()[-1])
    assert d["steps"] == 12 and d["value"] > 0
    assert d["allocator"]["device_allocs_in_timed_region"] == 0, d["allocator"]


def test_bench_dump_outputs_repeat_from_run_to_run(tmp_path):
    """bench.py --dump-outputs: the last timed step's loss, network output, weights and gradient (seeded samples) as float
    .npy files under 64 MB, and two runs with the same arguments dump the same values (the untimed steps before the timed
    region follow a fixed schedule, so the last timed step sees the same weights, optimizer state and inputs)."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    dumps = []
    for k in range(2):
        d = tmp_path / ("run%d" % k)
        cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2", "--batch", "4",
               "--classes", "3", "--size", "160", "--support", "160", "--dump-outputs", str(d)]
        out = subprocess.run(cmd, cwd=root, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-2000:]
        line = json.loads(out.stdout.strip().splitlines()[-1])
        assert line["steps"] == 3 and line["ms_per_step"] > 0 and "cpu_baseline" not in line and "also_measured" not in line
        files = sorted(os.listdir(str(d)))
        assert files == ["grad_sample.npy", "loss.npy", "output.npy", "weights_sample.npy"], files
        assert sum(os.path.getsize(str(d / f)) for f in files) < 64 << 20
        arrs = {f: np.load(str(d / f)) for f in files}
        assert all(a.dtype in (np.float32, np.float64) and np.isfinite(a).all() for a in arrs.values())
        assert arrs["output.npy"].shape == (4 * 3, 30, 5, 5)
        dumps.append(arrs)
    for f, a in dumps[0].items():
        assert np.allclose(a, dumps[1][f], rtol=1e-5, atol=1e-6), f
