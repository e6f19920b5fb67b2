"""bench.py's own multi-rank launcher (``--gpus N`` without torchrun): the parent starts N ranks
under torch.distributed.run before anything touches a GPU, rank 0 prints ONE JSON line with
n_gpus = N and global_batch = N*B, and the gathered u0 equals an unsharded solve.  Run here over
gloo with the CPU solver stub (tests/bench_stub.py) standing in for the HIP handle."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench_cmd(workload, gpus, batch, steps, extra=()):
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get('PYTHONPATH', ''),
               OMP_NUM_THREADS='1')
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT', 'BENCH_STUB_STALL_RANK'):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(REPO, 'bench.py'), '--gpus', str(gpus),
           '--steps', str(steps), '--warmup', '1', '--workload', workload,
           '--batch', str(batch), '--no-cpu-baseline', '--backend', 'gloo',
           '--solver-stub', 'tests.bench_stub'] + list(extra)
    return cmd, env


def _run_bench(tmp_path, workload, gpus, batch, steps=2, extra=()):
    dump = str(tmp_path / f'gather_{workload}.npy')
    cmd, env = _bench_cmd(workload, gpus, batch, steps, list(extra) + ['--dump-gather', dump])
    p = subprocess.run(cmd, cwd=REPO, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-4000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0]), np.load(dump)


@pytest.mark.parametrize('workload,gpus,batch', [('c2', 2, 12), ('c5', 2, 10)])
def test_bench_gpus_n_launches_n_ranks(tmp_path, workload, gpus, batch):
    from oracle.inputs import make_inputs
    from oracle.ocp import OcpSpec, mpc_solve
    line, got = _run_bench(tmp_path, workload, gpus, batch)
    assert line['n_gpus'] == gpus
    assert line['config']['global_batch'] == gpus * batch
    assert line['value'] > 0 and line['bad_status'] == 0
    N = 20 if workload == 'c2' else 40
    inp = make_inputs(workload, ids=np.arange(gpus * batch, dtype=np.uint64), N=N)
    ref = mpc_solve(inp['x0'], inp['xref'], inp['uref'], OcpSpec(N=N), wind=inp['wind'])['u0']
    if workload == 'c2':   # the RCCL/gloo all-gather of u0 in global id order
        assert got.shape == (gpus * batch, 4)
        assert np.array_equal(got, ref)
    else:                  # the all-reduced per-motor histogram
        b = np.clip(np.floor(ref * (64 / 65.0)), 0, 63).astype(np.int64)
        want = np.stack([np.bincount(b[:, m], minlength=64) for m in range(4)])
        assert np.array_equal(got, want)


def test_bench_gpus_1_runs_in_process(tmp_path):
    line, got = _run_bench(tmp_path, 'c2', 1, 8, steps=1)
    assert line['n_gpus'] == 1 and line['config']['global_batch'] == 8
    assert got.shape == (8, 4)


def test_bench_plain_run_is_lean_and_dumps_the_last_step(tmp_path):
    """Without --full the line is the headline alone (no roofline, secondary, latency or CPU
    baseline blocks), --steps is the number of timed steps, and --dump-outputs writes what the last
    timed step returned: u0, X, U and status of every instance, equal to the oracle's solve."""
    from oracle.inputs import make_inputs
    from oracle.ocp import OcpSpec, mpc_solve
    d = tmp_path / 'outs'
    line, _ = _run_bench(tmp_path, 'c2', 1, 6, steps=3, extra=['--dump-outputs', str(d)])
    for k in ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step'):
        assert k in line
    for k in ('roofline', 'secondary', 'latency_b1', 'cpu_baseline'):
        assert k not in line
    assert line['steps'] == 3
    assert line['value'] == pytest.approx(6 * 1e3 / line['ms_per_step'], rel=1e-9)
    assert sorted(p.name for p in d.iterdir()) == ['U.npy', 'X.npy', 'status.npy', 'u0.npy']
    inp = make_inputs('c2', ids=np.arange(6, dtype=np.uint64), N=20)
    ref = mpc_solve(inp['x0'], inp['xref'], inp['uref'], OcpSpec(N=20))
    for name, shape in (('u0', (6, 4)), ('X', (6, 21, 12)), ('U', (6, 20, 4))):
        got = np.load(str(d / f'{name}.npy'))
        assert got.dtype == np.float64 and got.shape == shape
        assert np.array_equal(got, ref[name])
    st = np.load(str(d / 'status.npy'))
    assert st.dtype == np.float64 and np.array_equal(st, np.zeros(6))


def test_dump_outputs_samples_large_outputs(tmp_path):
    """Above 64 MB the per-instance arrays keep one seeded sample of rows, the same in every run."""
    import torch
    import bench

    class Pipe:
        mode, gathered, last = 'gather', None, 0
        outs = [(torch.arange(40.0, dtype=torch.float32).reshape(10, 4), None, None,
                 torch.zeros(10, dtype=torch.int32))]
    old = bench.DUMP_MAX_BYTES
    # room for 5 of the 10 rows (u0 fp32, status as fp64) and the two files' .npy headers
    bench.DUMP_MAX_BYTES = 5 * (4 * 4 + 8) + 2 * 256
    try:
        bench.dump_outputs(str(tmp_path / 'a'), Pipe)
        bench.dump_outputs(str(tmp_path / 'b'), Pipe)
        assert sum(p.stat().st_size for p in (tmp_path / 'a').iterdir()) <= bench.DUMP_MAX_BYTES
    finally:
        bench.DUMP_MAX_BYTES = old
    a, b = np.load(str(tmp_path / 'a' / 'u0.npy')), np.load(str(tmp_path / 'b' / 'u0.npy'))
    assert a.dtype == np.float32 and a.shape == (5, 4) and np.array_equal(a, b)
    rows = (a[:, 0] / 4).astype(int)
    assert np.all(np.diff(rows) > 0) and np.array_equal(a, Pipe.outs[0][0].numpy()[rows])
    assert np.load(str(tmp_path / 'a' / 'status.npy')).shape == (5,)


@pytest.mark.gpu
def test_bench_dump_outputs_on_the_gpu(tmp_path):
    """The HIP path's plain run: two runs with the same arguments dump identical arrays, and they
    match the fp64 oracle on the same seeded instances (the bound of smoke(): 1e-9 relative)."""
    from oracle.inputs import make_inputs
    from oracle.ocp import OcpSpec, mpc_solve
    outs = []
    for tag in ('a', 'b'):
        d = tmp_path / tag
        cmd = [sys.executable, os.path.join(REPO, 'bench.py'), '--gpus', '1', '--steps', '2', '--warmup', '1',
               '--batch', '96', '--dump-outputs', str(d)]
        p = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stderr[-4000:]
        line = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith('{')][-1])
        assert line['steps'] == 2 and line['bad_status'] == 0 and 'roofline' not in line
        outs.append({n: np.load(str(d / f'{n}.npy')) for n in ('u0', 'X', 'U', 'status')})
    inp = make_inputs('c2', ids=np.arange(96, dtype=np.uint64), N=20)
    ref = mpc_solve(inp['x0'], inp['xref'], inp['uref'], OcpSpec(N=20))
    for n in ('u0', 'X', 'U'):
        assert outs[0][n].dtype == np.float64
        assert np.array_equal(outs[0][n], outs[1][n])
        err = np.abs(outs[0][n] - ref[n]).max() / max(np.abs(ref[n]).max(), 1.0)
        assert err < 1e-9, (n, err)
    assert not outs[0]['status'].any()


def test_bench_gpus_4_adds_the_c4_secondary(tmp_path):
    """At 4 ranks the line also times BASELINE configs[3] (c4: input box, instance-sharded over 4
    GPUs); the gathered c4 u0 equals the unsharded oracle's active-set solution."""
    from oracle.inputs import make_inputs
    from oracle.ocp import OcpSpec, mpc_solve
    sb = 3
    line, _ = _run_bench(tmp_path, 'c2', 4, 4, steps=1, extra=['--full', '--secondary-batch', str(sb)])
    assert line['n_gpus'] == 4 and line['config']['global_batch'] == 16
    sec = line['secondary']
    assert sec['workload'].startswith('c4') and sec['global_batch'] == 4 * sb and sec['n_gpus'] == 4
    assert sec['value'] > 0 and sec['bad_status'] == 0
    assert 'active_set' in sec['roofline']
    got = np.load(str(tmp_path / 'gather_c2.npy') + '.secondary.npy')
    inp = make_inputs('c4', ids=np.arange(4 * sb, dtype=np.uint64), N=30)
    ref = mpc_solve(inp['x0'], inp['xref'], inp['uref'],
                    OcpSpec(N=30, lbu=np.zeros(4), ubu=np.full(4, 65.0)))['u0']
    assert got.shape == (4 * sb, 4)
    assert np.array_equal(got, ref)


def test_bench_gpus_8_adds_the_c5_histogram_secondary(tmp_path):
    """At 8 ranks the line also times BASELINE configs[4] (c5: N = 40, fp32, wind, instance-sharded
    over 8 GPUs with only the u0* histogram reduced, bench.py sec_name): the all-reduced per-motor
    histogram equals the global oracle histogram of all 8 shards' instances, bit for bit."""
    from oracle.inputs import make_inputs
    from oracle.ocp import OcpSpec, mpc_solve
    sb = 3
    line, _ = _run_bench(tmp_path, 'c2', 8, 2, steps=1, extra=['--full', '--secondary-batch', str(sb)])
    assert line['n_gpus'] == 8 and line['config']['global_batch'] == 16
    sec = line['secondary']
    assert sec['workload'].startswith('c5') and sec['global_batch'] == 8 * sb and sec['n_gpus'] == 8
    assert sec['value'] > 0 and sec['bad_status'] == 0
    got = np.load(str(tmp_path / 'gather_c2.npy') + '.secondary.npy')
    inp = make_inputs('c5', ids=np.arange(8 * sb, dtype=np.uint64), N=40)
    ref = mpc_solve(inp['x0'], inp['xref'], inp['uref'], OcpSpec(N=40), wind=inp['wind'])['u0']
    b = np.clip(np.floor(ref * (64 / 65.0)), 0, 63).astype(np.int64)
    want = np.stack([np.bincount(b[:, m], minlength=64) for m in range(4)])
    assert got.shape == (4, 64) and got.sum() == 4 * 8 * sb
    assert np.array_equal(got, want)


def test_bench_stalled_rank_fails_fast():
    """A rank that never joins the rendezvous: the others give up after --init-timeout and the
    parent exits non-zero well before the driver's limit (no hang, no JSON line)."""
    import time
    cmd, env = _bench_cmd('c2', 2, 4, 1, ['--init-timeout', '8'])
    env['BENCH_STUB_STALL_RANK'] = '1'
    t0 = time.time()
    p = subprocess.run(cmd, cwd=REPO, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode != 0
    assert not [ln for ln in p.stdout.splitlines() if ln.startswith('{')]
    assert time.time() - t0 < 200
