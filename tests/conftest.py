"""Shared pytest configuration.

Markers:
  gpu — tests that need a real MI355X; run with ``pytest -m gpu`` on a
        GPU box, excluded in CPU CI via ``-m "not gpu"``.
"""

import faulthandler
import os
import pathlib
import shutil
import stat
import sys
import tempfile

import pytest

REPO_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO_ROOT not in sys.path:
    sys.path.insert(0, REPO_ROOT)


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: requires an MI355X GPU")
    config.addinivalue_line(
        "markers", "timeout(seconds): per-test watchdog override")


# Plugin-independent per-test watchdog. pytest-timeout is configured in
# pyproject.toml, but round 1's driver-side GPU run burned its whole
# 1200 s budget inside one wedged fixture without the plugin ever
# firing (plugin autoload can be disabled in the harness env), so this
# conftest arms faulthandler's C-level watchdog around every test
# protocol (fixtures included): on expiry it dumps every thread's stack
# and exits the process — a wedge costs minutes, not the lease.
_WATCHDOG_OFF = os.environ.get("OIM_TEST_NO_WATCHDOG") == "1"


def _watchdog_seconds(item):
    marker = item.get_closest_marker("timeout")
    if marker and marker.args:
        return float(marker.args[0])
    return 300.0


@pytest.hookimpl(hookwrapper=True)
def pytest_runtest_protocol(item, nextitem):
    if _WATCHDOG_OFF or not hasattr(faulthandler, "dump_traceback_later"):
        yield
        return
    faulthandler.dump_traceback_later(_watchdog_seconds(item), exit=True)
    try:
        yield
    finally:
        faulthandler.cancel_dump_traceback_later()


def _short_tmp_root():
    """The system temp dir when its path is short, else /tmp."""
    root = tempfile.gettempdir()
    return root if len(root) <= 16 else "/tmp"


@pytest.fixture
def tmp_path():
    """A short per-test directory, replacing pytest's own ``tmp_path``.

    Nearly every test binds unix sockets (hipstored, vhost controllers,
    gRPC endpoints) below this directory, and AF_UNIX paths are limited
    to 107 chars. pytest's default
    ``<tmpdir>/pytest-of-<user>/pytest-N/<test name>0`` overflows that
    under a long temp dir, user name or test name; the daemon then
    refuses to start.
    """
    path = tempfile.mkdtemp(prefix="oim-", dir=_short_tmp_root())
    yield pathlib.Path(path)
    shutil.rmtree(path, ignore_errors=True)


@pytest.fixture(scope="session")
def _mknod_permitted():
    """Whether this process may create block device nodes (CAP_MKNOD)."""
    probe_dir = tempfile.mkdtemp(prefix="oim-", dir=_short_tmp_root())
    try:
        os.mknod(os.path.join(probe_dir, "probe"), stat.S_IFBLK | 0o600,
                 os.makedev(1, 3))
        return True
    except PermissionError:
        return False
    finally:
        shutil.rmtree(probe_dir, ignore_errors=True)


@pytest.fixture
def mknod_calls(_mknod_permitted, monkeypatch):
    """Let the CSI remote backend "create" device nodes unprivileged.

    With CAP_MKNOD the real ``os.mknod`` runs and the list stays empty.
    Without it, ``os.mknod`` is replaced for the test by a recorder that
    appends ``(path, mode, device)`` and leaves a plain file at ``path``,
    so tests check the arguments at the syscall boundary instead of the
    node's ``st_rdev``.
    """
    calls = []
    if not _mknod_permitted:
        def fake_mknod(path, mode=0o600, device=0):
            calls.append((path, mode, device))
            with open(path, "xb"):
                pass

        monkeypatch.setattr(os, "mknod", fake_mknod)
    return calls


@pytest.fixture
def tmp_sock(tmp_path):
    """A short unix socket path (AF_UNIX limit is 107 chars)."""
    path = tmp_path / "s.sock"
    return str(path)
