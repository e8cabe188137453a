"""CPU-side checks of v_diffusion.metrics.fid_score: it imports without a GPU, the VDIFF_NATIVE_FID=1 opt-in of the star-import
surface, the no-download rule of get_precomputed, how model=None resolves, and the argument checks that run before any device
work.  Every check runs in a fresh interpreter (environment variables read at import, patched network entry points, a reference
tree loaded under the v_diffusion_ref alias)."""
import os
import subprocess
import sys
import textwrap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "v-diffusion-torch_amd")
NATIVE = ["Manifold", "ManifoldBuilder", "calc_pr"]
FID = ["InceptionStatistics", "calc_fd", "get_precomputed"]


def _run(body, *args, reference=None, native_fid=False):
    """run `body` in a fresh interpreter with the package importable; sys.argv[1:] = args; returns its stdout lines"""
    env = {k: v for k, v in os.environ.items() if k not in ("VDIFF_REFERENCE_ROOT", "VDIFF_NATIVE_FID")}
    if reference is not None:
        env["VDIFF_REFERENCE_ROOT"] = str(reference)
    if native_fid:
        env["VDIFF_NATIVE_FID"] = "1"
    code = f"import sys\nsys.path[:0] = [{PKG!r}, {ROOT!r}]\n" + textwrap.dedent(body)
    r = subprocess.run([sys.executable, "-c", code, *map(str, args)], capture_output=True, text=True, env=env, cwd=ROOT, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return r.stdout.splitlines()


def _fake_reference(root):
    """a reference tree whose metrics package holds a stub Inception network and stub FID names"""
    pkg = root / "v_diffusion"
    (pkg / "metrics").mkdir(parents=True)
    (pkg / "__init__.py").write_text("")
    (pkg / "metrics" / "__init__.py").write_text("from .fid_score import InceptionStatistics, get_precomputed, calc_fd\n")
    (pkg / "metrics" / "fid_score.py").write_text(
        "class InceptionStatistics:\n    pass\n\ndef get_precomputed(*a):\n    return 'pre'\n\ndef calc_fd(*a):\n    return 'fd'\n")
    (pkg / "metrics" / "inception.py").write_text(
        "import torch\n\n"
        "class InceptionV3(torch.nn.Module):\n"
        "    BLOCK_INDEX_BY_DIM = {64: 0, 192: 1, 768: 2, 2048: 3}\n\n"
        "    def __init__(self, output_blocks):\n"
        "        super().__init__()\n"
        "        self.output_blocks = list(output_blocks)\n")


_STAR = """
from v_diffusion.metrics import *
names = sorted(n for n in dir() if not n.startswith('_') and n != 'sys')
print(names)
print([globals()[n].__module__ for n in ('InceptionStatistics', 'calc_fd', 'get_precomputed') if n in names])
"""


def test_module_imports_without_a_gpu_and_the_package_stays_lazy():
    assert _run("""
        import v_diffusion
        print('v_diffusion.metrics' in sys.modules)
        import v_diffusion.metrics.fid_score as F
        print(sorted(n for n in ('InceptionStatistics', 'calc_fd', 'calculate_frechet_distance', 'get_precomputed') if hasattr(F, n)))
    """) == ["False", str(["InceptionStatistics", "calc_fd", "calculate_frechet_distance", "get_precomputed"])]


def test_native_fid_opt_in_lists_six_native_names(tmp_path):
    mod = "v_diffusion.metrics.fid_score"
    assert _run(_STAR, native_fid=True) == [str(sorted(NATIVE + FID)), str([mod] * 3)]
    _fake_reference(tmp_path)                                    # the opt-in wins over a checkout
    assert _run(_STAR, native_fid=True, reference=tmp_path) == [str(sorted(NATIVE + FID)), str([mod] * 3)]


def test_default_surface_is_unchanged(tmp_path):
    assert _run(_STAR) == [str(NATIVE), "[]"]
    _run("""
        import pytest
        import v_diffusion.metrics as M
        with pytest.raises(ImportError, match="VDIFF_REFERENCE_ROOT"):
            M.calc_fd
    """)
    _fake_reference(tmp_path)
    assert _run(_STAR, reference=tmp_path) == [str(sorted(NATIVE + FID)), str(["v_diffusion_ref.metrics.fid_score"] * 3)]


def test_get_precomputed_never_reaches_the_network(tmp_path):
    _run("""
        import os
        import urllib.request
        import numpy as np
        import pytest
        import requests
        from v_diffusion.metrics import fid_score as F

        def no_network(*a, **k):
            raise AssertionError("network access attempted")
        requests.get = no_network
        urllib.request.urlopen = no_network
        d = sys.argv[1]
        with pytest.raises(FileNotFoundError) as e:
            F.get_precomputed("cifar10", download_dir=d)
        assert os.path.join(d, "fid_stats_cifar10_train.npz") in str(e.value) and "http" in str(e.value)
        assert os.listdir(d) == []
        mu, sigma = np.arange(4.0), np.eye(4)
        np.savez(os.path.join(d, "fid_stats_cifar10_train.npz"), mu=mu, sigma=sigma)
        m, s = F.get_precomputed("cifar10", download_dir=d)
        assert np.array_equal(m, mu) and np.array_equal(s, sigma)
        np.savez(os.path.join(d, "fid_stats_celeba_148x148.npz"), mu=mu + 1, sigma=sigma)
        assert np.array_equal(F.get_precomputed("celeba", d)[0], mu + 1) and np.array_equal(F.get_precomputed("cropped_celeba", d)[0], mu + 1)
        with pytest.raises(KeyError):
            F.get_precomputed("no_such_set", d)
    """, tmp_path)


def test_model_none_needs_the_reference_and_builds_its_network(tmp_path):
    _run("""
        import pytest
        from v_diffusion.metrics import fid_score as F
        with pytest.raises(ImportError, match="VDIFF_REFERENCE_ROOT"):
            F.InceptionStatistics()
        with pytest.raises(ImportError, match="VDIFF_REFERENCE_ROOT"):
            F.InceptionStatistics(model=None, activation_dim=64, device="cpu")
    """)
    _fake_reference(tmp_path)
    _run("""
        import torch
        from v_diffusion.metrics import fid_score as F
        s = F.InceptionStatistics.__new__(F.InceptionStatistics)        # the model-building path only: no device on this tier
        torch.nn.Module.__init__(s)
        for dim, block in ((2048, 3), (192, 1)):
            s.activation_dim = dim
            net = s.load_model()
            assert type(net).__module__ == "v_diffusion_ref.metrics.inception" and net.output_blocks == [block]
    """, reference=tmp_path)


def test_argument_checks_before_device_work():
    _run("""
        import numpy as np
        import pytest
        import torch
        from v_diffusion.metrics import fid_score as F
        mu, s = np.zeros(32), np.eye(32)
        with pytest.raises(ValueError, match="mean vectors"):
            F.calc_fd(mu, s, np.zeros(16), s)
        with pytest.raises(ValueError, match="covariances"):
            F.calc_fd(mu, s, mu, np.eye(16))
        with pytest.raises(ValueError, match="covariances"):
            F.calc_fd(np.zeros(16), s, np.zeros(16), s)
        with pytest.raises(ValueError, match="multiples of 16"):
            F.calculate_frechet_distance(np.zeros(24), np.eye(24), np.zeros(24), np.eye(24))
        with pytest.raises(RuntimeError, match="no CPU path"):
            F.calculate_frechet_distance(mu, s, mu, s, device="cpu")
        net = torch.nn.Identity()
        with pytest.raises(RuntimeError, match="no CPU path"):
            F.InceptionStatistics(model=net, activation_dim=64, device="cpu")
        with pytest.raises(RuntimeError, match="no CPU path"):
            F.InceptionStatistics(model=net, activation_dim=64, device=torch.device("cpu"))
        with pytest.raises(ValueError, match="activation_dim"):
            F.InceptionStatistics(model=net, activation_dim=100, device="cpu")
    """)
