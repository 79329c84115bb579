"""The default schedule of a handle against the hardware queues the HIP runtime was started with (egdst_host.inc: eg_default_groups,
build_schedule; include/egdst.h: egdst_set_groups), on the CPU harness without a sanitizer and without a GPU.  GPU_MAX_HW_QUEUES is
read from the environment when a handle is created, so every setting runs in a child process of its own
(tests/cpu_emu/run_emu_schedule.py: a small C2 form, one cell per draw)."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))

# cells per period on both sides of every threshold of the rule
CELLS = [63, 64, 511, 512, 1023, 1024]


def documented_groups(hwq, cells):
    """include/egdst.h, egdst_set_groups: the default number of regular groups"""
    if hwq >= 10:
        return 16 if cells >= 1024 and hwq >= 20 else 8 if cells >= 512 else 4 if cells >= 64 else 1
    return 4 if cells >= 1024 else 1


SETTINGS = ['unset', '4', '8', '9', '10', '24']   # (9 and 10: either side of the seam between the rule's two branches)


@pytest.fixture(scope='module')
def schedules():
    """{setting: [(cells, groups and lanes at create, groups, lanes and stragglers after a solve)]}, the children side by side"""
    env = {k: v for k, v in os.environ.items() if k not in ('GPU_MAX_HW_QUEUES', 'EGDST_GROUPS', 'EGDST_ADAPTIVE')}
    script = os.path.join(HERE, 'cpu_emu', 'run_emu_schedule.py')
    # (the first child builds the harness library; the others find it)
    first = subprocess.run([sys.executable, script, 'unset'], env=env, capture_output=True, text=True, timeout=900)
    assert first.returncode == 0, first.stderr[-3000:]
    procs = {q: subprocess.Popen([sys.executable, script, q] + [str(c) for c in CELLS], env=env, stdout=subprocess.PIPE,
                                 stderr=subprocess.PIPE, text=True) for q in SETTINGS}
    out = {}
    for q, p in procs.items():
        so, se = p.communicate(timeout=900)
        assert p.returncode == 0, se[-3000:]
        rows = [[int(x) for x in ln.split() if x.lstrip('-').isdigit()] for ln in so.splitlines() if ln.startswith('cells ')]
        assert [r[0] for r in rows] == CELLS, so
        out[q] = rows
    return out


@pytest.mark.parametrize('setting', SETTINGS)
def test_default_groups_are_the_documented_ones(schedules, setting):
    hwq = 4 if setting == 'unset' else int(setting)   # (unset: the HIP runtime's own default)
    for cells, g0, l0, g1, _, _ in schedules[setting]:
        assert g0 == documented_groups(hwq, cells), (setting, cells, g0)
        # lanes come from a solve's history; these solves regenerate no guess stream, so the count stays the default
        assert l0 == 0 and g1 == g0


@pytest.mark.parametrize('setting', SETTINGS)
def test_streams_that_need_a_queue_fit_the_queues_the_rule_leaves(schedules, setting):
    """Group 0 runs on the handle's stream; groups 1 .. and the straggler lanes each need a queue of their own.  A lane is handed out
    only where a queue is left beside the groups' and the null stream's, so lanes never exceed hwq - 1 - groups."""
    hwq = 4 if setting == 'unset' else int(setting)
    for cells, _, _, g, lanes, stragglers in schedules[setting]:
        assert 0 <= lanes <= max(0, hwq - 1 - g), (setting, cells, g, lanes)
        assert lanes <= stragglers
        if hwq >= 10:
            assert (g - 1) + lanes <= hwq - 2, (setting, cells, g, lanes)
