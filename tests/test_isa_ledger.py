"""Static instruction ledger of the fused c2 kernel (tools/isa_ledger.py): the recompiled kernel
may not grow past the entry committed in profiles/isa_c2.json, and that entry is below the parent's
in both of the kernel's main loops.  Host only: cross-compiles for gfx950, runs nothing on a GPU."""
import json
import os
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'tools'))
import isa_ledger  # noqa: E402

pytestmark = [pytest.mark.slow,
              pytest.mark.skipif(not isa_ledger.have_hipcc(), reason='hipcc not found')]

# one SIMD's share of the CU's LDS (mpcb_capi.hip LDS_PER_WAVE_SIMD): one wave per SIMD must fit
LDS_PER_WAVE_SIMD = 160 * 1024 // 4


@pytest.fixture(scope='module')
def committed():
    return json.load(open(os.path.join(REPO, 'profiles', 'isa_c2.json')))


@pytest.fixture(scope='module')
def current():
    return isa_ledger.ledger()


def test_committed_result_is_below_parent(committed):
    for name in ('rollout', 'riccati'):
        new, old = isa_ledger.role(committed['result'], name), isa_ledger.role(committed['parent'], name)
        print(name, old['total'], '->', new['total'])
        assert new['total'] < old['total']
    assert committed['result']['meta']['scratch'] == 0
    assert committed['result']['meta']['vgpr_spill'] == 0


def test_recompiled_kernel_within_committed_entry(committed, current):
    ref = committed['result']
    assert current['kernel'] == ref['kernel']
    for name in ('rollout', 'riccati'):
        now, was = isa_ledger.role(current, name), isa_ledger.role(ref, name)
        print(name, now['total'], 'committed', was['total'])
        assert now['total'] <= was['total']
    assert current['meta']['scratch'] <= ref['meta']['scratch'] == 0
    assert current['meta']['vgpr_spill'] == 0
    assert current['meta']['lds'] <= ref['meta']['lds'] <= LDS_PER_WAVE_SIMD
