import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


@pytest.fixture
def sock_dir(tmp_path):
    """A directory for a test's Unix-domain sockets.  A socket's whole path must fit AF_UNIX's sun_path (108 bytes, NUL
    included); pytest's tmp_path under a deep temporary directory need not leave room for it, so a short-named directory
    under /tmp is taken instead when it would not."""
    import shutil
    import tempfile
    from pathlib import Path

    if len(str(tmp_path)) + len("/inquistr-4294967295-dev0.sock") < 100:
        yield tmp_path
        return
    d = tempfile.mkdtemp(prefix="inq", dir="/tmp")
    try:
        yield Path(d)
    finally:
        shutil.rmtree(d, ignore_errors=True)


@pytest.fixture(scope="session")
def kat():
    import json

    with open(os.path.join(ROOT, "tests", "golden", "kat_call.json")) as f:
        return json.load(f)


@pytest.fixture(scope="session")
def orc():
    """The C oracle (test infrastructure)."""
    from oracle import orc as _orc

    _orc.build()
    return _orc
