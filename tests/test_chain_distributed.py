"""Chains that carry posterior moments through parallelHMCSampler's all-gather (gloo, world size 2, CPU): with keep_samples=False
every rank ends with every chain's moments, and a chain's block is 2 nparam + O(nsamples) doubles."""
import os
import socket
import sys

import numpy as np

from tests.conftest import ROOT

NS, BURN = 6, 2


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _stub_samples(c, nparam):
    return np.random.default_rng([7, c]).standard_normal((nparam, NS)) * (1.0 + 0.3 * c) + c


def _moments(x):
    return x.shape[1], x.mean(axis=1), ((x - x.mean(axis=1, keepdims=True)) ** 2).sum(axis=1)


def _worker(rank, world, port, nchains, q):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    from hmcmt2d_amd import sampler
    from hmcmt2d_amd.structs import HMCPrior, HMCStatus
    from tests.helpers import make_problem
    dist.init_process_group("gloo", rank=rank, world_size=world)
    mesh, data, inv, m = make_problem("tiny")
    nparam, ndata = len(inv.strModel), len(inv.obsData)

    def run_chain(c, rng):
        """what runHMCSampler(device_chain=True, keep_samples=False) returns: no sample column, the first data column, the moments"""
        acc = np.array([True, False, True, c % 2 == 0, True, False])
        st = HMCStatus(int(acc.sum()), int((~acc).sum()), acc, rng.standard_normal((4, NS + 1)))
        st.moments = _moments(_stub_samples(c, nparam)[:, BURN:])
        return np.zeros((nparam, 0)), st, (rng.standard_normal((ndata, 1)) + 1j * rng.standard_normal((ndata, 1)))

    sent = []
    gather = dist.all_gather_into_tensor

    def spy(recv, send, *a, **k):
        sent.append(send.numel())
        return gather(recv, send, *a, **k)

    dist.all_gather_into_tensor = spy
    hm, hs, hd = sampler.parallelHMCSampler(mesh, data, inv, HMCPrior(totalsamples=NS, burninsamples=BURN), nchains=nchains, seed=11,
                                            run_chain=run_chain, keep_samples=False)
    dist.all_gather_into_tensor = gather
    per = (nchains + world - 1) // world
    merged = sampler.mergeMoments([s.moments for s in hs])
    rhat = sampler.gelmanRubin([s.moments for s in hs]) if nchains > 1 else None
    q.put((rank, [s.moments for s in hs], merged, rhat, sent[0] // per, [x.shape for x in hm], [x.shape for x in hd],
           [s.nAccept for s in hs], (nparam, ndata)))
    dist.destroy_process_group()


def _spawn(nchains):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, nchains, q)) for r in range(2)]
    for p in procs:
        p.start()
    out = sorted((q.get(timeout=180) for _ in procs), key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    return out


def test_every_rank_ends_with_every_chains_moments():
    nchains = 3
    out = _spawn(nchains)
    nparam, ndata = out[0][8]
    for rank, moments, merged, rhat, blk, mshapes, dshapes, nacc, _ in out:
        for c in range(nchains):
            n, mean, m2 = _moments(_stub_samples(c, nparam)[:, BURN:])
            assert moments[c][0] == n == NS - BURN
            assert np.array_equal(moments[c][1], mean) and np.array_equal(moments[c][2], m2)
        allx = np.concatenate([_stub_samples(c, nparam)[:, BURN:] for c in range(nchains)], axis=1)
        n, mean, m2 = _moments(allx)
        assert merged[0] == n == nchains * (NS - BURN)
        assert np.abs(merged[1] - mean).max() <= 1e-13 * np.abs(mean).max() and np.all(np.abs(merged[2] - m2) <= 1e-13 * m2)
        from hmcmt2d_amd.sampler import gelmanRubin
        assert np.array_equal(rhat, gelmanRubin([_moments(_stub_samples(c, nparam)[:, BURN:]) for c in range(nchains)]))
        assert mshapes == [(nparam, 0)] * nchains and dshapes == [(ndata, 1)] * nchains
        assert nacc == [4, 3, 4]
        # the block of one chain, as parallelHMCSampler's docstring states it for keep_samples=False
        assert blk == 2 * nparam + 5 * NS + 2 * ndata + 7
        assert blk < nparam * NS
    assert all(np.array_equal(out[0][3], o[3]) for o in out)


def test_a_rank_without_a_chain_takes_the_block_layout_from_the_others():
    """one chain on two ranks: rank 1 runs none, and neither `keep_samples` nor `device_chain` tells it that the stub's blocks carry
    moments -- the ranks agree on the layout before the gather, and both end with the chain's moments"""
    (r0, r1) = _spawn(1)
    nparam, ndata = r0[8]
    n, mean, m2 = _moments(_stub_samples(0, nparam)[:, BURN:])
    for rank, moments, merged, rhat, blk, mshapes, dshapes, nacc, _ in (r0, r1):
        assert moments[0][0] == n and np.array_equal(moments[0][1], mean) and np.array_equal(moments[0][2], m2)
        assert mshapes == [(nparam, 0)] and dshapes == [(ndata, 1)] and nacc == [4]
        assert blk == 2 * nparam + 5 * NS + 2 * ndata + 7
