"""The kernel names the bf16 launchers report (tests/parity_cases.py: the instantiation tables) are kernels of the
gfx950 code object of the built library: timers, the benchmark's roofline and the profiles are keyed on them."""

import pathlib
import re
import shutil
import subprocess

import pytest

import parity_cases as P

LLVM = pathlib.Path("/opt/rocm/lib/llvm/bin")


def _device_kernels(lib: pathlib.Path, tmp: pathlib.Path) -> set:
    """Demangled kernel symbols of the library's gfx950 code objects, namespaces and the parameter list stripped (as
    tools/kernel_resources.py prints them), all whitespace removed."""
    objcopy, bundler, readelf = (LLVM / t for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf"))
    if not all(t.exists() for t in (objcopy, bundler, readelf)) or shutil.which("c++filt") is None:
        pytest.fail("the LLVM binary tools of the ROCm toolchain are needed to read the code object")
    fat = tmp / "fat.bin"
    subprocess.check_call([str(objcopy), f"--dump-section=.hip_fatbin={fat}", str(lib), str(tmp / "host.so")])
    magic, blob, mangled = b"__CLANG_OFFLOAD_BUNDLE__", fat.read_bytes(), []
    starts = [m.start() for m in re.finditer(magic, blob)]   # one bundle per translation unit
    for k, (lo, hi) in enumerate(zip(starts, starts[1:] + [len(blob)])):
        one, co = tmp / f"unit{k}.bin", tmp / f"unit{k}.co"
        one.write_bytes(blob[lo:hi])
        subprocess.check_call([str(bundler), "--unbundle", "--type=o", f"--input={one}",
                               "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"], stderr=subprocess.DEVNULL)
        notes = subprocess.run([str(readelf), "--notes", str(co)], capture_output=True, text=True, check=True).stdout
        mangled += re.findall(r"^\s*\.name:\s+(\S+)$", notes, flags=re.M)
    dem = subprocess.run(["c++filt"], input="\n".join(mangled), capture_output=True, text=True, check=True).stdout
    names = set()
    for line in dem.splitlines():
        line = re.sub(r"\(anonymous namespace\)::|gnntrk::", "", line)
        depth, cut = 0, len(line)
        for i, ch in enumerate(line):   # the parameter list starts at the first '(' outside the template arguments
            depth += (ch == "<") - (ch == ">")
            if ch == "(" and depth == 0:
                cut = i
                break
        names.add(re.sub(r"\s+", "", line[:cut]).removeprefix("void"))
    return names


def test_reported_kernel_names_exist(tmp_path):
    from gnn_tracking_amd import _build

    kernels = _device_kernels(_build.build_lib(), tmp_path)
    assert len(kernels) > 400, len(kernels)
    wanted = {n for _, names in P.BF16_FWD_INSTANTIATIONS for n in names}
    wanted |= {a[0] for _, answers in P.BF16_BWD_INSTANTIATIONS for a in answers}
    # the shapes of the default models, as profiler output quotes them
    for must in ("mlp16_fwd_kernel<1, 3, true, false, 4, true>",
                 "mlp16_bwd_kernel<1, 3, 2, true, false, 2, IoRelational<3, false> >",
                 "mlp16_bwd_kernel<1, 3, 2, true, false, 2, IoRelational<2, false> >",
                 "mlp16_bwd_kernel<1, 3, 1, true, false, 2, IoObject>",
                 "mlp16_bwd_kernel<1, 3, 2, true, true, 2, IoHeadT<false> >",
                 "mlp16_bwd_kernel<1, 3, 0, false, false, 2, IoEncoder8<1> >"):
        assert must in wanted, must
    missing = sorted(n for n in wanted if re.sub(r"\s+", "", n) not in kernels)
    assert not missing, missing
