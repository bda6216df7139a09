"""Every A/B route switch of the native library (tests/route_switches.py) against the oracle / the reference's
logits, and -- where the table says so -- bit for bit against the run it is compared with.

Each case runs tests/route_switch_child.py in a fresh interpreter (the switches are read once per process) with the parent's
environment plus the row's switch; the child asserts the workloads' own bars.  The parent then checks that the switch really
changed what ran (the kernel names, grids and counts the profiler saw differ from the base run's on the row's ``acts_on``
workloads; equal where the row expects no effect) and, for ``bits`` rows, that every output equals the base run's bits.  The
base runs (no switch, or the row's ``base``) are made once per workload and cached for the module.

Children run one at a time.  A child that dies on a signal or times out ends the run: every later case fails naming it."""
import collections
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from route_switches import ROWS, row_id

pytestmark = pytest.mark.gpu

CHILD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "route_switch_child.py")
TIMEOUT = 600


@pytest.fixture(scope="module")
def runner(tmp_path_factory):
    root = tmp_path_factory.mktemp("route_switches")
    done = {}                                       # (env key, workload) -> output directory
    state = {"dead": None}

    def run(case, env, workloads):
        """outputs of `workloads` under `env`: {workload: dir}; base runs are cached"""
        if state["dead"]:
            pytest.fail(f"not run: child of case {state['dead']} died earlier in this run")
        key = tuple(sorted(env.items()))
        todo = [w for w in workloads if (key, w) not in done]
        if todo:
            d = root / f"run{len(os.listdir(root)):03d}"
            d.mkdir()
            try:
                r = subprocess.run([sys.executable, CHILD, str(d), ",".join(todo)], env=dict(os.environ, **env),
                                   capture_output=True, text=True, timeout=TIMEOUT)
            except subprocess.TimeoutExpired:
                state["dead"] = case
                pytest.fail(f"{case}: child timed out after {TIMEOUT} s ({env}, {todo}); no further children are started")
            if r.returncode < 0:
                state["dead"] = case
                pytest.fail(f"{case}: child died on signal {-r.returncode} ({env}, {todo}); no further children are started\n"
                            f"{r.stdout[-2000:]}\n{r.stderr[-3000:]}")
            assert r.returncode == 0, (case, env, todo, r.stdout[-2000:], r.stderr[-4000:])
            for w in todo:
                assert f"ok {w} " in r.stdout, (case, w, r.stdout[-2000:])
                done[(key, w)] = d / w
        return {w: done[(key, w)] for w in workloads}

    return run


def _kernels(d):
    with open(os.path.join(d, "kernels.json")) as f:
        return collections.Counter(json.dumps(k) for k in json.load(f))


def _arrays(d):
    return {n[:-4]: np.load(os.path.join(d, n)) for n in sorted(os.listdir(d)) if n.endswith(".npy")}


@pytest.mark.parametrize("row", ROWS, ids=[row_id(r) for r in ROWS])
def test_route_switch(runner, row):
    case = row_id(row)
    base = runner(case + " (base)", row["base"], row["workloads"])
    got = runner(case, dict(row["base"], **row["env"]), row["workloads"])
    for w in row["workloads"]:
        kb, kg = _kernels(base[w]), _kernels(got[w])
        assert sum(kb.values()) > 0, (case, w, "the profiler saw no kernel launches")
        if w in row["acts_on"]:
            diff = sorted((kg - kb).elements())[:8], sorted((kb - kg).elements())[:8]
            assert kg != kb, (case, w, "the switch did not change the launched kernels: its route was not taken")
            print(case, w, "new:", diff[0], "gone:", diff[1])
        elif not row["acts_on"]:
            assert kg == kb, (case, w, "a switch that must change nothing changed the launches",
                              sorted((kg - kb).elements())[:8], sorted((kb - kg).elements())[:8])
        if row["relation"] == "bits":
            ab, ag = _arrays(base[w]), _arrays(got[w])
            assert ab.keys() == ag.keys(), (case, w)
            for n in ab:
                assert ab[n].shape == ag[n].shape and ab[n].tobytes() == ag[n].tobytes(), (
                    case, w, n, "not bit-identical", int((ab[n] != ag[n]).sum()))
