"""ls_set_tuning's accept / reject table (no launch, runs without a GPU), and: the host dispatch
does not depend on the environment -- the variables that once selected a diagnostics build,
A/B switches and tuning keys change no ops.conv_path answer."""
import json
import os
import subprocess
import sys


from latentsync_amd import _lib, ops

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# every live key with its default value (include/ls_hip.h)
DEFAULTS = {1: 0, 2: 0, 3: 0, 4: 0, 6: 1, 7: 1, 8: 1, 9: 0, 12: 1, 13: 0, 15: 1, 16: 1, 17: 1, 18: 1, 19: 1, 20: 0}
ACCEPTED = [(k, v) for k in (1, 6, 7, 8, 13, 15, 16, 18, 19, 20) for v in (0, 1)] + \
           [(2, v) for v in (0, 1, 2, 3, 4, 5, 6, 9)] + [(3, 0), (3, 2), (4, 0), (4, 8), (9, 0), (12, 1), (17, 1)]
REFUSED = [(k, v) for k in (0, 5, 10, 11, 14, 21, -1) for v in (0, 1)] + \
          [(2, 7), (2, 8), (2, 10), (2, -1), (9, 1), (12, 0), (17, 2), (17, 0), (17, 3), (5, 32), (5, 64)]


def test_accept_reject_table():
    lib = _lib.load()
    try:
        for k, v in ACCEPTED:
            assert lib.ls_set_tuning(k, v) == 0, f"key {k} = {v} refused: {lib.ls_last_error().decode()}"
        for k, v in REFUSED:
            assert lib.ls_set_tuning(k, v) != 0, f"key {k} = {v} accepted"
            assert "diagnostics" not in lib.ls_last_error().decode()
    finally:
        for k, v in DEFAULTS.items():
            assert lib.ls_set_tuning(k, v) == 0


def _conv_path_answers():
    """Every ops.conv_path answer of tests/test_conv_dispatch.py, in call order."""
    import test_conv_dispatch as T
    answers, real = [], ops.conv_path

    def recording(*a, **kw):
        answers.append(real(*a, **kw))
        return answers[-1]

    ops.conv_path = recording
    try:
        for name in sorted(n for n in dir(T) if n.startswith("test_")):
            try:
                getattr(T, name)()
            except AssertionError:
                pass  # (the answers are compared below; test_conv_dispatch.py itself asserts them)
    finally:
        ops.conv_path = real
    return answers


_CHILD = """
import json, sys
sys.path[:0] = [{repo!r}, {tests!r}]
import test_tuning_keys as K
print("ANSWERS " + json.dumps(K._conv_path_answers()))
"""


def test_environment_does_not_reach_the_dispatch():
    clean = _conv_path_answers()
    assert len(clean) >= 8 and 3 in clean
    env = dict(os.environ, LS_DIAG_BUILD="1", LS_UPS_PHASE="0", LS_GN_EPILOGUE="0", LS_HALO="0", LS_TUNE="8=0")
    r = subprocess.run([sys.executable, "-s", "-c", _CHILD.format(repo=REPO, tests=os.path.join(REPO, "tests"))],
                       cwd=REPO, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    lines = [l for l in r.stdout.splitlines() if l.startswith("ANSWERS ")]
    assert len(lines) == 1, r.stdout + r.stderr
    assert json.loads(lines[0][len("ANSWERS "):]) == clean
