"""The occupancy condition the overlapped tail of bnmf_gibbs_run rests on (no GPU needed: hipcc cross-compiles and reports
per kernel).

One GPU: the relayout, Gram and end-of-iteration kernels (post_kernel, gram_reduce_kernel, finish_kernel) run on a second
stream BESIDE the contraction (api.hip: TailOverlap).  The contraction's grid is one block per CU in one round, one wave per
SIMD, so a tail kernel that does not fit into what that wave leaves of the SIMD's registers, wave slots and the CU's LDS waits
until the contraction's blocks retire -- all together -- and runs behind it, as if there were no second stream.  Every parity
test stays green when that happens; only the benchmark gets slower.  A later edit to a shared helper can do it, so the
condition is asserted here, from the compiler's own resource remarks and the block sizes the launch code uses."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bnmtf_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

# gfx950 (CDNA4): a SIMD lane has 512 registers, vector and accumulation registers of a wave in one allocation (vector part
# rounded up, granule 8); 8 wave slots per SIMD, 4 SIMDs and 160 KiB of LDS per CU
REGS_PER_SIMD, WAVE_SLOTS, SIMDS, LDS_PER_CU, GRANULE = 512, 8, 4, 160 * 1024, 8

# the contraction instances of the Gibbs workloads: K = 64 (headline) and K <= 32, four 32-column tiles per wave
GEMMS = ["gemm_bf16x3_kernelILi2ELi3ELi4ELi1EE", "gemm_bf16x3_kernelILi1ELi3ELi4ELi1EE"]
# (translation unit, substring of the mangled name, the constant its launch passes as the block size, the pattern of that launch)
TAIL = [
    ("kernel_post.hip", "post_kernelILb0EE", "kPostThreads", r"hipLaunchKernelGGL\(post_kernel<false>, dim3\(nblk, 2\), dim3\((\w+)\)"),
    ("kernel_post.hip", "18gram_reduce_kernelE", "kGramReduceThreads", r"hipLaunchKernelGGL\(gram_reduce_kernel, dim3\(\(ps \+ 31\) / 32 \+ extra\), dim3\((\w+)\)"),
    ("kernel_misc.hip", "13finish_kernelE", "kFinishThreads", r"hipLaunchKernelGGL\(finish_kernel, dim3\(1\), dim3\((\w+)\)"),
]


def _up(v, m):
    return (v + m - 1) // m * m


def _resources(tu):
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I" + os.path.join(ROOT, "include"),
           "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, tu), "-o", os.devnull]
    return subprocess.Popen(cmd, cwd=CSRC, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


def _parse(out):
    found, name = {}, None
    for line in out.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1); found[name] = {}
            continue
        m = re.search(r"remark:\s+(VGPRs Spill|SGPRs Spill|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]): (\d+)", line)
        if m and name:
            found[name][m.group(1)] = int(m.group(2))
    return found


def _block_sizes():
    """threads per block of the three tail kernels: the constant named in each launch (kernel_post.hip, kernel_misc.hip), its
    value from kernels.h"""
    hdr = open(os.path.join(CSRC, "kernels.h")).read()
    consts = {}
    for decl in re.findall(r"constexpr int ([^;]*);", hdr):
        for name, val in re.findall(r"(\w+) = (\d+)", decl):
            consts[name] = int(val)
    sizes = {}
    for tu, sub, const, pat in TAIL:
        m = re.search(pat, open(os.path.join(CSRC, tu)).read())
        assert m, "launch of %s not found in %s" % (sub, tu)
        assert m.group(1) == const and const in consts, (sub, m.group(1))
        sizes[sub] = consts[const]
    return sizes


def _one(found, sub):
    hits = [(n, r) for n, r in found.items() if sub in n]
    assert len(hits) == 1, (sub, sorted(found))
    return hits[0]


@pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.exists(HIPCC), reason="no hipcc")
def test_tail_kernels_fit_beside_a_contraction_wave():
    procs = {tu: _resources(tu) for tu in ["kernel_gemm.hip"] + sorted({t for t, _, _, _ in TAIL})}
    found = {}
    for tu, p in procs.items():
        out = p.communicate(timeout=900)[0]
        assert p.returncode == 0, out[-2000:]
        found[tu] = _parse(out)
    sizes = _block_sizes()
    for gsub in GEMMS:
        gname, g = _one(found["kernel_gemm.hip"], gsub)
        assert g["VGPRs Spill"] == 0 and g["ScratchSize [bytes/lane]"] == 0, (gname, g)
        gemm_regs = _up(g["VGPRs"], GRANULE) + g["AGPRs"]          # one wave per SIMD (256-thread blocks, one block per CU)
        free_regs = REGS_PER_SIMD - gemm_regs
        free_lds = LDS_PER_CU - g["LDS Size [bytes/block]"]
        assert free_regs > 0 and free_lds > 0, (gname, g)
        for tu, sub, _, _ in TAIL:
            name, r = _one(found[tu], sub)
            threads = sizes[sub]
            assert threads % 64 == 0 and threads <= 1024, (name, threads)
            waves_per_simd = -(-(threads // 64) // SIMDS)
            regs = waves_per_simd * _up(r["VGPRs"] + r["AGPRs"], GRANULE)
            print("%s beside %s: %d threads, %d waves/SIMD x %d registers = %d of %d free; LDS %d of %d free" % (
                sub, gsub, threads, waves_per_simd, _up(r["VGPRs"] + r["AGPRs"], GRANULE), regs, free_regs, r["LDS Size [bytes/block]"], free_lds))
            assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["ScratchSize [bytes/lane]"] == 0, (name, r)
            assert regs <= free_regs, (name, r, threads, gname, g)
            assert 1 + waves_per_simd <= WAVE_SLOTS, (name, threads)
            assert 2 * r["LDS Size [bytes/block]"] <= free_lds, (name, r, gname, g)      # ... and a second block of itself


def test_finish_block_is_eight_waves():
    """finish_kernel's sums are one per wave, waves 0-7 (kernel_misc.hip): the block is exactly those"""
    assert _block_sizes()["13finish_kernelE"] == 8 * 64
