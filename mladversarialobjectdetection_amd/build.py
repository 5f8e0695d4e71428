"""Build libphx.so in-tree for gfx950 (hipcc; no CMake).  `python -m mladversarialobjectdetection_amd.build`"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


def build(jobs: int = 8, verbose: bool = False) -> str:
    csrc = os.path.join(HERE, "csrc")
    env = dict(os.environ)
    cmd = ["make", "-C", csrc, f"-j{min(jobs, 16)}"]
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if verbose or r.returncode != 0:
        sys.stdout.write(r.stdout)
    if r.returncode != 0:
        raise RuntimeError("libphx build failed")
    # the kernel parity checkers link against the library (tests/test_gpu_gemm_kernels.py,
    # tests/test_gpu_conv_kernels.py, tests/test_gpu_norm_kernels.py, tests/test_gpu_conv3_kernels.py, tests/test_gpu_eot_kernels.py, tests/test_gpu_post_kernels.py, tests/test_gpu_unet_kernels.py and tests/test_gpu_batch_invariance.py run them)
    # (tests/kernels_sefold: the checker of the SE backward without its dx tensor, tests/test_gpu_sefold_kernels.py)
    # (tests/kernels_nms_seg: the checker of the segmented NMS and its host-only teeth program,
    # tests/test_gpu_nms_modes_kernels.py, tests/test_nms_modes_host.py)
    # (tests/kernels_boxloss: the checker of the box-regression term's kernels and its host-only teeth program,
    # tests/test_gpu_boxloss_kernels.py, tests/test_idiou_oracle.py)
    for sub in ("kernels", "kernels_sefold", "kernels_nms_seg", "kernels_boxloss"):
        kern = os.path.join(os.path.dirname(HERE), "tests", sub)
        if not os.path.isfile(os.path.join(kern, "Makefile")):
            continue
        r = subprocess.run(["make", "-C", kern, f"-j{min(jobs, 16)}"], env=env, stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, text=True)
        if verbose or r.returncode != 0:
            sys.stdout.write(r.stdout)
        if r.returncode != 0:
            raise RuntimeError(f"tests/{sub} build failed")
    return os.path.join(HERE, "libphx.so")


if __name__ == "__main__":
    print(build(verbose=True))
