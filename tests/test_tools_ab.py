"""tools/ab.py, the A/B timer of library variants: which children it starts.  A library whose child exited non-zero is not started
again, and after an exit status that means a GPU fault, an abort or a time limit nothing more is started at all.  (The children
here are stand-ins that only log their library's name and exit: no GPU, no library.)"""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = ("import os, sys\n"
        "n = os.path.basename(os.environ['NTG_AMD_LIB'])\n"
        "open(os.environ['AB_LOG'], 'a').write(n + '\\n')\n"
        "print('ran', n)\n"
        "k = 'AB_DO_' + n.replace('.', '_')\n"
        "if os.environ.get(k) == 'sleep':\n"
        "    import time; time.sleep(60)\n"
        "if os.environ.get(k) == 'kill':\n"
        "    import signal; os.kill(os.getpid(), signal.SIGKILL)\n"
        "if os.environ.get(k) == 'fault':\n"
        "    sys.stderr.write('RuntimeError: HIP error: an illegal memory access was encountered\\n'); sys.exit(1)\n"
        "sys.exit(int(os.environ.get('AB_RC_' + n.replace('.', '_'), '0')))\n")


@pytest.fixture
def ab(monkeypatch, tmp_path):
    spec = importlib.util.spec_from_file_location("ab_tool", os.path.join(ROOT, "tools", "ab.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    monkeypatch.setattr(mod, "CHILD", FAKE)
    log = tmp_path / "started.txt"
    monkeypatch.setenv("AB_LOG", str(log))
    mod.started = lambda: log.read_text().split() if log.exists() else []
    return mod


def test_every_library_twice_when_all_is_well(ab):
    assert ab.main(["a.so", "b.so"]) == 0
    assert ab.started() == ["a.so", "b.so", "a.so", "b.so"]


def test_failed_library_is_dropped(ab, monkeypatch):
    monkeypatch.setenv("AB_RC_b_so", "3")
    assert ab.main(["a.so", "b.so", "c.so"]) == 1
    assert ab.started() == ["a.so", "b.so", "c.so", "a.so", "c.so"]


@pytest.mark.parametrize("rc", [134, 139, 124, 137])
def test_nothing_starts_after_a_fault(ab, monkeypatch, rc):
    monkeypatch.setenv("AB_RC_b_so", str(rc))
    assert ab.main(["a.so", "b.so", "c.so"]) == rc
    assert ab.started() == ["a.so", "b.so"]


def test_nothing_starts_after_a_kill(ab, monkeypatch):
    monkeypatch.setenv("AB_DO_b_so", "kill")
    assert ab.main(["a.so", "b.so", "c.so"]) == 128 + 9
    assert ab.started() == ["a.so", "b.so"]


def test_nothing_starts_after_a_fault_met_as_an_exception(ab, monkeypatch):
    monkeypatch.setenv("AB_DO_b_so", "fault")   # exit status 1, the fault's text on stderr
    assert ab.main(["a.so", "b.so", "c.so"]) == 139
    assert ab.started() == ["a.so", "b.so"]


def test_nothing_starts_after_the_time_limit(ab, monkeypatch):
    monkeypatch.setattr(ab, "LIMIT_S", 1)   # (the stand-in would sleep a minute: it is killed after this second)
    monkeypatch.setenv("AB_DO_b_so", "sleep")
    assert ab.main(["a.so", "b.so", "c.so"]) == 124
    assert ab.started() == ["a.so", "b.so"]
