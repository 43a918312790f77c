"""Host-side checks of the guided matcher's C ABI: the version, the two exported entries and their argument checks (which return before any launch)."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from accelerated_features_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def test_version_303_and_the_guided_entries(lib):
    from accelerated_features_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "xfeat_hip.h")).read()
    assert int(re.search(r"#define XFH_VERSION (\d+)", hdr).group(1)) == 303 == lib.xfh_version()
    raw = C.CDLL(_lib.LIB_PATH)
    for name in ("xfh_match_guided_workspace_bytes", "xfh_match_mnn_guided"):
        assert hasattr(raw, name) and name in _lib.SIGNATURES
    assert re.search(r"#define XFH_GUIDE_FUNDAMENTAL 0", hdr) and re.search(r"#define XFH_GUIDE_HOMOGRAPHY +1", hdr)
    assert (_lib.GUIDE_FUNDAMENTAL, _lib.GUIDE_HOMOGRAPHY) == (0, 1)


def test_workspace_size_and_argument_errors(lib):
    P, N1, N2 = 32, 4096, 4096
    nb = lib.xfh_match_guided_workspace_bytes(P, N1, N2)
    assert nb >= P * (N1 + N2) * (8 + 16) and nb % 256 == 0        # keys + gate constants
    assert lib.xfh_match_guided_workspace_bytes(0, N1, N2) == 0 and lib.xfh_match_guided_workspace_bytes(P, -1, N2) == 0
    x = C.c_void_p(256)                                             # never dereferenced: every call below fails its argument checks first

    def call(d1=x, models=x, kind=0, thr=3.0, P=1, N1=8, N2=8, ps=512, ws=x, ws_bytes=1 << 20):
        return lib.xfh_match_mnn_guided(d1, ps, x, 512, x, 16, x, 16, None, None, 0, 0, P, N1, N2, models, kind, thr, -1.0, x, x, x, ws, ws_bytes, None)

    for kw in (dict(d1=None), dict(models=None), dict(kind=2), dict(kind=-1), dict(thr=0.0), dict(thr=-3.0), dict(thr=float('nan')), dict(thr=float('inf')),
               dict(P=0), dict(N1=0), dict(P=70000), dict(ps=514), dict(ws=None), dict(ws_bytes=16)):
        assert call(**kw) != 0, kw
        assert lib.xfh_last_error()
