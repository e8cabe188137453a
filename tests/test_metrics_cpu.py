"""CPU-side checks of v_diffusion.metrics: the star-import surface with and without a reference checkout, the Manifold pickle
path, the no-download rule of VGGFeatureExtractor and the argument checks that run before any device work.

Every check runs in a fresh interpreter: loading a reference tree under the v_diffusion_ref alias, patching torch.hub / urllib and
drawing from torch's global generator then leave no state behind in the process that runs the rest of the suite."""
import os
import subprocess
import sys
import textwrap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "v-diffusion-torch_amd")
NATIVE = ["Manifold", "ManifoldBuilder", "calc_pr"]
ALL = sorted(NATIVE + ["InceptionStatistics", "calc_fd", "get_precomputed"])


def _run(body, *args, reference=None):
    """run `body` in a fresh interpreter with the package importable; sys.argv[1:] = args; returns its stdout lines"""
    env = {k: v for k, v in os.environ.items() if k != "VDIFF_REFERENCE_ROOT"}
    if reference is not None:
        env["VDIFF_REFERENCE_ROOT"] = str(reference)
    code = f"import sys\nsys.path[:0] = [{PKG!r}, {ROOT!r}]\n" + textwrap.dedent(body)
    r = subprocess.run([sys.executable, "-c", code, *map(str, args)], capture_output=True, text=True, env=env, cwd=ROOT, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return r.stdout.splitlines()


def _fake_reference(root):
    """a reference tree whose metrics package exports the reference's six names (FID ones as stubs)"""
    pkg = root / "v_diffusion"
    (pkg / "metrics").mkdir(parents=True)
    (pkg / "__init__.py").write_text("from .utils import seed_all\n")
    (pkg / "utils.py").write_text("def seed_all(s):\n    return s\n")
    (pkg / "metrics" / "__init__.py").write_text(
        "from .fid_score import InceptionStatistics, get_precomputed, calc_fd\n"
        "__all__ = ['InceptionStatistics', 'get_precomputed', 'calc_fd']\n")
    (pkg / "metrics" / "fid_score.py").write_text(
        "class InceptionStatistics:\n    pass\n\ndef get_precomputed(*a):\n    return 'pre'\n\ndef calc_fd(*a):\n    return 'fd'\n")


_STAR = """
from v_diffusion.metrics import *
print(sorted(n for n in dir() if not n.startswith('_') and n != 'sys'))
print('calc_fd' in dir() and calc_fd() == 'fd')
"""


def test_star_import_lists_three_names_without_a_reference_and_six_with_one(tmp_path):
    assert _run(_STAR)[:2] == [str(NATIVE), "False"]
    _fake_reference(tmp_path)
    assert _run(_STAR, reference=tmp_path)[:2] == [str(ALL), "True"]


def test_delegated_names_need_the_reference(tmp_path):
    _run("""
        import pytest
        import v_diffusion.metrics as M
        with pytest.raises(ImportError, match="VDIFF_REFERENCE_ROOT"):
            M.calc_fd
        with pytest.raises(AttributeError):
            M.no_such_metric
    """)
    _fake_reference(tmp_path)
    _run("""
        import v_diffusion.metrics as M
        assert M.get_precomputed() == "pre" and M.InceptionStatistics.__module__ == "v_diffusion_ref.metrics.fid_score"
        assert M.ManifoldBuilder.__module__ == "v_diffusion.metrics.precision_recall"
    """, reference=tmp_path)


def test_importing_the_package_does_not_import_metrics():
    assert _run("import v_diffusion\nprint('v_diffusion.metrics' in sys.modules)") == ["False"]


def test_saved_manifold_loads_with_a_plain_torch_load(tmp_path):
    _run("""
        import torch
        from v_diffusion.metrics import Manifold, ManifoldBuilder
        b = ManifoldBuilder.__new__(ManifoldBuilder)            # the saving path only: no kernels on this tier
        g = torch.Generator().manual_seed(0)
        b.features = torch.randn(6, 5, generator=g).half()
        b.kth = torch.rand(6, generator=g).half()
        path = sys.argv[1] + "/sub/pr_manifold_x.pt"
        b.save(path)
        m = torch.load(path)
        assert type(m) is Manifold
        assert type(m).__module__ + "." + type(m).__qualname__ == "v_diffusion.metrics.precision_recall.Manifold"
        assert torch.equal(m.features, b.features) and torch.equal(m.kth, b.kth) and m.kth.dtype == torch.float16
    """, tmp_path)


def test_vgg_extractor_never_downloads(tmp_path):
    _run("""
        import os
        import urllib.request
        import pytest
        import torch.hub
        from v_diffusion.metrics import precision_recall as pr
        torch.hub.set_dir(sys.argv[1])

        def no_network(*a, **k):
            raise AssertionError("network access attempted")
        torch.hub.download_url_to_file = no_network
        urllib.request.urlopen = no_network
        with pytest.raises(FileNotFoundError) as e:
            pr.VGGFeatureExtractor()
        assert os.path.join(sys.argv[1], "vgg16.pt") in str(e.value) and pr.VGGFeatureExtractor.WEIGHTS_URL in str(e.value)
    """, tmp_path)


def test_argument_checks_before_device_work():
    _run("""
        import pytest
        import torch
        from v_diffusion.metrics import Manifold, ManifoldBuilder, calc_pr
        f = torch.randn(20, 8, generator=torch.Generator().manual_seed(0)).half()
        with pytest.raises(ValueError, match="nhood_size"):
            ManifoldBuilder(features=f, nhood_size=16)
        with pytest.raises(RuntimeError, match="no CPU path"):
            ManifoldBuilder(features=f, nhood_size=3, device="cpu")
        with pytest.raises(RuntimeError, match="no CPU path"):
            calc_pr(Manifold(f, f[:, 0]), Manifold(f, f[:, 0]), 10000, 10000, torch.device("cpu"))
    """)


def test_to_uint8_matches_the_reference_rule():
    assert _run("""
        import torch
        from v_diffusion.metrics.precision_recall import to_uint8
        print(to_uint8(torch.tensor([-1.5, -1.0, -0.5, 0.0, 0.3, 0.99, 1.0, 2.0])).tolist())
    """) == [str([0, 0, 64, 128, 166, 254, 255, 255])]
