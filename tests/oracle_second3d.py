"""fp64 / fp32 CPU evaluations of the full-size LiDAR trunk (tests/ref_second3d.py on ``synth.SECOND3D_CASES['full']``:
[1,128,8,100,100], layer_nums [5,5,5]) in the process pool of tests/oracle_jobs.py, next to the GPU tests.

oracle_jobs' workers look jobs up by key in THEIR copy of ``oracle_jobs.JOBS``, which does not know this module, so the jobs are
submitted here with a function of this module that returns what ``oracle_jobs._run`` returns ((result, seconds)); the futures are
put where ``oracle_jobs.get`` looks for them, and the keys are entered in ``oracle_jobs.JOBS`` of this process so that ``get``
evaluates inline when there is no pool (one test run by hand, COOCC_ORACLE_POOL=0).  Measured: 8 s in fp64, 2 s in fp32."""
import os
import time

import torch

import oracle_jobs
import co_occ_amd.synth as synth

import ref_second3d

KEYS = {"second3d_full_o64": torch.float64, "second3d_full_o32": torch.float32}


def full_case():
    c = synth.SECOND3D_CASES["full"]
    bcfg, ncfg = synth.second3d_cfg(c["layer_nums"])
    b, n = ref_second3d.build(bcfg, ncfg)
    sdb, sdn = synth.second3d_weights(b, n, c["seed"])
    return bcfg, ncfg, sdb, sdn, synth.second3d_input(c["grid_zyx"], seed=c["seed"])


def job_full(which):
    """(the three backbone outputs, the neck output) [B,C,Z,Y,X] of the restatement in the key's precision."""
    bcfg, ncfg, sdb, sdn, x = full_case()
    b, n = ref_second3d.build(bcfg, ncfg, sdb, sdn, KEYS[which])
    feats, y = ref_second3d.run(b, n, x)
    return list(feats), y


def _run(which):
    t = time.time()
    with torch.no_grad():
        out = job_full(which)
    return out, time.time() - t


for _k in KEYS:
    oracle_jobs.JOBS[_k] = (job_full, (_k,), 10)


def start():
    """Submit both evaluations to oracle_jobs' pool (created here the way ``oracle_jobs.start`` does when conftest did not)."""
    keys = [k for k in KEYS if k not in oracle_jobs._FUT and k not in oracle_jobs._DONE]
    if not keys or os.environ.get("COOCC_ORACLE_POOL", "1") == "0":
        return
    if oracle_jobs._POOL is None:
        import multiprocessing as mp
        from concurrent.futures import ProcessPoolExecutor
        ncpu = oracle_jobs._usable_cores()
        threads = 4 if ncpu >= 8 else 2
        oracle_jobs._POOL = ProcessPoolExecutor(max_workers=max(1, min(len(keys), (ncpu - 2) // threads)), mp_context=mp.get_context("spawn"),
                                                initializer=oracle_jobs._init_worker, initargs=(threads,))
    for k in keys:
        oracle_jobs._FUT[k] = oracle_jobs._POOL.submit(_run, k)
        oracle_jobs._T0[k] = time.time()


def get(which):
    return oracle_jobs.get(which)
