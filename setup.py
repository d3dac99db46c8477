"""Build the xgboost_ray_amd package + its gfx950 HIP extension in-tree.

Usage:
    PYTORCH_ROCM_ARCH=gfx950 python setup.py build_ext --inplace
"""

import os
import sys

from setuptools import find_packages, setup

ext_modules = []
cmdclass = {}

if "--cpu-only" not in sys.argv:
    try:
        from torch.utils import cpp_extension

        os.environ.setdefault("PYTORCH_ROCM_ARCH", "gfx950")
        src_dir = os.path.join(
            os.path.dirname(os.path.abspath(__file__)), "xgboost_ray_amd", "csrc"
        )
        sources = [
            os.path.join(src_dir, f)
            for f in sorted(os.listdir(src_dir))
            if f.endswith((".cpp", ".hip"))
            and not f.endswith("_hip.hip")  # hipify build artifacts
        ]
        if sources:
            ext_modules = [
                cpp_extension.CUDAExtension(
                    name="xgboost_ray_amd._hip_ops",
                    sources=sources,
                    extra_compile_args={
                        "cxx": ["-O3", "-std=c++17"],
                        # -ffp-contract=off: the double-precision split
                        # scan must be bitwise-identical to the CPU torch
                        # oracle (FMA contraction flips near-tie splits);
                        # the hot histogram path is integer and unaffected.
                        "nvcc": ["-O3", "-std=c++17", "-ffp-contract=off"],
                    },
                ),
                # The ranking kernels are a module of their own: the one
                # above keeps its build line, and so its generated code.
                # This one opts out of packed-fp32 (v_pk_*_f32) selection;
                # its float32 work is comparisons and one store per row.
                cpp_extension.CUDAExtension(
                    name="xgboost_ray_amd._hip_rank_ops",
                    sources=[os.path.join(src_dir, "rank", "rank_ops.hip")],
                    extra_compile_args={
                        "cxx": ["-O3", "-std=c++17"],
                        # -ffp-contract=off: the AP prefix sums must be the
                        # bits of a sequential float64 cumsum
                        "nvcc": ["-O3", "-std=c++17", "-ffp-contract=off",
                                 "-Xclang", "-target-feature",
                                 "-Xclang", "-packed-fp32-ops"],
                    },
                ),
                # The multiclass kernels, again a module of their own with
                # the same opt-out: their float32 work is one weight
                # multiply per value and the maxima.
                cpp_extension.CUDAExtension(
                    name="xgboost_ray_amd._hip_softmax_ops",
                    sources=[os.path.join(src_dir, "multi",
                                          "softmax_ops.hip")],
                    extra_compile_args={
                        "cxx": ["-O3", "-std=c++17"],
                        # -ffp-contract=off: a row's float64 steps are the
                        # contract's, none fused with its neighbour
                        "nvcc": ["-O3", "-std=c++17", "-ffp-contract=off",
                                 "-Xclang", "-target-feature",
                                 "-Xclang", "-packed-fp32-ops"],
                    },
                ),
                # The survival kernels (AFT, Cox), a module of their own
                # with the same flags: their float32 work is the weight
                # multiply and the maxima.
                cpp_extension.CUDAExtension(
                    name="xgboost_ray_amd._hip_survival_ops",
                    sources=[os.path.join(src_dir, "survival",
                                          "survival_ops.hip")],
                    extra_compile_args={
                        "cxx": ["-O3", "-std=c++17"],
                        # -ffp-contract=off: a row's float64 steps and the
                        # scans' adds are the contract's, none fused
                        "nvcc": ["-O3", "-std=c++17", "-ffp-contract=off",
                                 "-Xclang", "-target-feature",
                                 "-Xclang", "-packed-fp32-ops"],
                    },
                ),
                # The pointwise regression kernels, a module of their own
                # with the same flags.
                cpp_extension.CUDAExtension(
                    name="xgboost_ray_amd._hip_pointwise_ops",
                    sources=[os.path.join(src_dir, "pointwise",
                                          "pointwise_ops.hip")],
                    extra_compile_args={
                        "cxx": ["-O3", "-std=c++17"],
                        # -ffp-contract=off: the float32 gradients are the
                        # bits of torch's eager chain, one rounding per op
                        "nvcc": ["-O3", "-std=c++17", "-ffp-contract=off",
                                 "-Xclang", "-target-feature",
                                 "-Xclang", "-packed-fp32-ops"],
                    },
                ),
                # The multiclass AUC kernels, a module of their own with the
                # flags of the softmax module: their float32 work is the
                # row maximum.
                cpp_extension.CUDAExtension(
                    name="xgboost_ray_amd._hip_auc_ops",
                    sources=[os.path.join(src_dir, "auc", "auc_ops.hip")],
                    extra_compile_args={
                        "cxx": ["-O3", "-std=c++17"],
                        # -ffp-contract=off: a row's float64 steps are the
                        # contract's, p * n_bins not fused into a compare
                        "nvcc": ["-O3", "-std=c++17", "-ffp-contract=off",
                                 "-Xclang", "-target-feature",
                                 "-Xclang", "-packed-fp32-ops"],
                    },
                ),
                # The weighted quantile sketch kernels (tree_method="approx"),
                # a module of their own: integer sums only, so no float flag.
                cpp_extension.CUDAExtension(
                    name="xgboost_ray_amd._hip_sketch_ops",
                    sources=[os.path.join(src_dir, "sketch",
                                          "sketch_ops.hip")],
                    extra_compile_args={
                        "cxx": ["-O3", "-std=c++17"],
                        "nvcc": ["-O3", "-std=c++17"],
                    },
                ),
            ]
            cmdclass = {"build_ext": cpp_extension.BuildExtension}
    except Exception as e:  # pragma: no cover
        print(f"warning: HIP extension skipped: {e}", file=sys.stderr)
else:
    sys.argv.remove("--cpu-only")

setup(
    name="xgboost_ray_amd",
    version="0.1.0",
    description=(
        "MI355X-native distributed gradient-boosted-tree trainer with the "
        "capabilities of xgboost_ray"
    ),
    packages=find_packages(include=["xgboost_ray_amd", "xgboost_ray_amd.*"]),
    python_requires=">=3.9",
    ext_modules=ext_modules,
    cmdclass=cmdclass,
)
