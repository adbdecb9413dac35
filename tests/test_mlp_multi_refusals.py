"""What wh_mlp_forward_multi refuses, with no device: the symbol is declared and both libraries export
it, the host engine answers WH_ENOTSUP like its other wh_mlp_* entry points, and the gfx950 library
checks every argument rule of include/warehouse_amd.h -- in the header's order -- before it touches the
GPU, so dummy pointers are never dereferenced and a refused call launches nothing."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def nat():
    from warehouse import _native

    return _native


def job(nat, **kw):
    """A well-formed job on dummy pointers (a refused call dereferences nothing)."""
    f = dict(packed=0x10000, rows=5, obs=0x20000, xfrag=None, logits=0x30000, actions=0x40000, explore=0, step=0, seed=0)
    f.update(kw)
    return nat.WhMlpJob(**f)


def call(nat, lib, desc, jobs, n=None):
    table = (nat.WhMlpJob * max(len(jobs), 1))(*jobs)
    return lib.wh_mlp_forward_multi(ctypes.byref(desc) if desc is not None else None, len(jobs) if n is None else n,
                                    table, None)


def test_symbol_is_declared_and_exported_by_both_libraries(nat):
    assert "wh_mlp_forward_multi" in nat.SYMBOLS
    assert hasattr(nat.lib(), "wh_mlp_forward_multi") and hasattr(nat.host_lib(), "wh_mlp_forward_multi")
    assert nat.WH_MLP_MAX_JOBS == 8
    # the job struct as the header lays it out: 7 eight-byte fields with explore / step sharing one
    assert ctypes.sizeof(nat.WhMlpJob) == 64 and nat.WhMlpJob.seed.offset == 56 and nat.WhMlpJob.step.offset == 52


def test_host_engine_answers_enotsup_and_touches_nothing(nat):
    import torch

    desc = nat.WhMlpDesc(37, 256, 256, 9, nat.WH_MLP_BF16)
    bufs = [torch.full((512,), 0xA5, dtype=torch.uint8) for _ in range(4)]
    j = job(nat, packed=bufs[0].data_ptr(), obs=bufs[1].data_ptr(), logits=bufs[2].data_ptr(), actions=bufs[3].data_ptr(),
            rows=1)
    assert call(nat, nat.host_lib(), desc, [j]) == nat.WH_ENOTSUP
    assert call(nat, nat.host_lib(), desc, []) == nat.WH_ENOTSUP
    assert all(bool((b == 0xA5).all()) for b in bufs)


@pytest.mark.parametrize("precision", ["bf16", "f32"])
def test_refusals_of_the_device_library_need_no_device(nat, precision):
    lib = nat.lib()
    E, N, OK = nat.WH_EINVAL, nat.WH_ENOTSUP, nat.WH_OK
    f32 = precision == "f32"
    desc = nat.WhMlpDesc(82, 512, 512, 9, nat.WH_MLP_F32 if f32 else nat.WH_MLP_BF16)
    good = job(nat)
    # d, the shape, njobs and jobs -- in this order
    assert call(nat, lib, None, [good]) == E
    assert lib.wh_mlp_forward_multi(None, 99, None, None) == E
    for bad in (nat.WhMlpDesc(83, 512, 512, 9, 0), nat.WhMlpDesc(82, 512, 512, 8, 0), nat.WhMlpDesc(82, 512, 512, 9, 7),
                nat.WhMlpDesc(82, 512, 256, 9, nat.WH_MLP_F32)):
        assert call(nat, lib, bad, [good]) == N
        assert call(nat, lib, bad, [good], n=-1) == N          # the shape comes before njobs
    assert call(nat, lib, desc, [good], n=-1) == E
    assert call(nat, lib, desc, [good] * 8, n=9) == E
    assert lib.wh_mlp_forward_multi(ctypes.byref(desc), 1, None, None) == E
    # nothing to do
    assert lib.wh_mlp_forward_multi(ctypes.byref(desc), 0, None, None) == OK
    assert call(nat, lib, desc, [], n=0) == OK
    dead = job(nat, rows=0, packed=None, obs=None, logits=None, actions=None)   # rows == 0: nothing else is looked at
    assert call(nat, lib, desc, [dead]) == OK
    assert call(nat, lib, desc, [dead] * 8) == OK
    assert call(nat, lib, desc, [job(nat, rows=0, obs=0x20000, xfrag=0x50001)]) == OK
    # per job, at every position
    for pos in (0, 1, 7):
        def at(j):
            jobs = [job(nat, rows=0) for _ in range(8)]
            jobs[pos] = j
            return call(nat, lib, desc, jobs)
        assert at(job(nat, rows=-1)) == E
        assert at(job(nat, rows=-1, packed=None)) == E
        assert at(job(nat, packed=None)) == E
        assert at(job(nat, obs=None)) == E                          # no input
        assert at(job(nat, logits=None, actions=None)) == E         # no output
        assert at(job(nat, xfrag=0x50000)) == E                     # both inputs
        assert at(job(nat, obs=None, xfrag=0x50000, logits=None, actions=None)) == E   # no output before xfrag's rules
        assert at(job(nat, obs=None, xfrag=0x50008)) == N           # misaligned
        assert at(job(nat, obs=None, xfrag=0x50001)) == N
        if f32:                                                     # (on bf16 this job is well formed: never sent here)
            assert at(job(nat, obs=None, xfrag=0x50000)) == N
    # two live jobs writing one buffer
    a = job(nat)
    assert call(nat, lib, desc, [a, job(nat, actions=0x41000)]) == E             # logits shared
    assert call(nat, lib, desc, [a, job(nat, logits=0x31000)]) == E              # actions shared
    assert call(nat, lib, desc, [a, job(nat, rows=0), job(nat, logits=0x31000, actions=0x41000),
                                 job(nat, logits=None)]) == E                    # ... with a later one
    assert call(nat, lib, desc, [job(nat, rows=0), job(nat, rows=0)]) == OK      # dead jobs share freely
    # the header's order: every job's own rules come before the shared-pointer rule, wherever the
    # pair stands -- a shared pointer among the first jobs and a LATER job's own defect answer the defect
    shares = job(nat, actions=0x41000)                                           # job 0's logits
    assert call(nat, lib, desc, [a, shares, job(nat, obs=None, xfrag=0x50008, logits=0x32000, actions=0x42000)]) == N
    assert call(nat, lib, desc, [a, shares, job(nat, rows=0), job(nat, obs=None, xfrag=0x50001, logits=0x32000,
                                                                   actions=0x42000)]) == N
    assert call(nat, lib, desc, [a, shares, job(nat, rows=-1)]) == E
    assert call(nat, lib, desc, [job(nat, obs=None, xfrag=0x50008), a, shares]) == N   # ... and an earlier one's
    assert call(nat, lib, desc, [a, shares, job(nat, logits=0x32000, actions=0x42000)]) == E   # no defect: the pair
