"""Run-once code of the fused c2 kernel (tools/isa_ledger.py): everything of
row_riccati_kernel<false, true> outside its two main loops -- the straight-line prologues and
epilogue plus the input-staging loop of the row prologue -- is below the same sum of the parent
entry committed in profiles/isa_c2.json, in that file's result entry and in a recompile, and the
kernel spills no more scalar registers than the parent.  Host only: cross-compiles for gfx950,
runs nothing on a GPU."""
import json
import os
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'tools'))
import isa_ledger  # noqa: E402

pytestmark = [pytest.mark.slow,
              pytest.mark.skipif(not isa_ledger.have_hipcc(), reason='hipcc not found')]


def run_once(entry: dict) -> int:
    """Instructions outside the rollout and Riccati loops: the straight-line rest and every other
    loop (the staging loop of the row prologue)."""
    return entry['straight_line']['total'] + sum(e['total'] for e in entry['loops'] if 'role' not in e)


@pytest.fixture(scope='module')
def committed():
    return json.load(open(os.path.join(REPO, 'profiles', 'isa_c2.json')))


@pytest.fixture(scope='module')
def current():
    return isa_ledger.ledger()


def test_committed_run_once_code_is_below_parent(committed):
    new, old = run_once(committed['result']), run_once(committed['parent'])
    print('run-once instructions', old, '->', new)
    assert new < old
    assert committed['result']['meta']['sgpr_spill'] <= committed['parent']['meta']['sgpr_spill']


def test_recompiled_run_once_code_is_below_parent(committed, current):
    now, old = run_once(current), run_once(committed['parent'])
    print('run-once instructions', old, '->', now, 'sgpr spills', committed['parent']['meta']['sgpr_spill'],
          '->', current['meta']['sgpr_spill'])
    assert current['kernel'] == committed['parent']['kernel']
    assert now < old
    assert current['meta']['sgpr_spill'] <= committed['parent']['meta']['sgpr_spill']
