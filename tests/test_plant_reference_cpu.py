"""The plant step (qlamd_wholebody_forward_dynamics_batch), everything that needs no GPU: the numpy reference the GPU tests
compare against (tests/plant_reference.py) checked on its own, the export and the header's feature-test macro, and the new
kernel's registers and scratch against what DESIGN.md section 4.6c states."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import plant_reference as PR  # noqa: E402

CASES = (("trot", 48), ("static", 16))


@pytest.fixture(scope="module")
def solved(oracle):
    """Every case solved once: (state, i, nu, mask, solution) per robot."""
    out = []
    for gait, B in CASES:
        s, tau = PR.case_states(gait, B)
        for i in range(B):
            nu, mask = PR.nu_of(s, i), PR.mask_of(s["stance"][i])
            out.append((s, i, nu, mask, PR.solve(s["q"][i], s["base_quat"][i], nu, tau[i], mask), tau[i]))
    return out


def test_the_contact_jacobian_has_full_rank_in_every_case(solved):
    """sigma_min of the four-foot Jc bounds that of every subset of feet from below (dropping rows cannot lower it): the KKT
    matrix of every support mask is then regular, and its condition number is what the 1e-6 parity bar of the GPU tests was
    sized for (2.9e3 on these states)."""
    worst_sigma, worst_cond = np.inf, 0.0
    for s, i, nu, mask, r, _ in solved:
        sigma = np.linalg.svd(r["Jc"], compute_uv=False).min()
        assert sigma > 0.05, (i, sigma)
        worst_sigma, worst_cond = min(worst_sigma, sigma), max(worst_cond, np.linalg.cond(r["K"]))
    print("sigma_min(Jc) >= %.3f, cond(K) <= %.3g" % (worst_sigma, worst_cond))
    assert worst_cond < 1e4


def test_leg_fk_is_the_lever_arm_of_the_contact_jacobian(solved, oracle):
    for s, i, nu, mask, r, _ in solved[::7]:
        for l in range(4):
            p = oracle.leg_fk(l, s["q"][i][3 * l:3 * l + 3])[0]
            skew = r["Jc"][3 * l:3 * l + 3, 3:6]  # -[r]x
            assert np.abs(np.array([skew[1, 2], skew[2, 0], skew[0, 1]]) - p).max() < 1e-14
            assert np.abs(r["Jc"][3 * l:3 * l + 3, 6 + 3 * l:9 + 3 * l] - oracle.leg_jacobian(l, s["q"][i][3 * l:3 * l + 3])).max() < 1e-14


def test_gamma_does_not_depend_on_the_difference_step(solved):
    """J' qd by central differences: step 1e-5 against 2e-5 (truncation is O(step^2), rounding O(1e-16 / step))."""
    worst = 0.0
    for s, i, nu, mask, r, _ in solved:
        worst = max(worst, np.abs(PR.gamma(s["q"][i], nu, 2e-5) - r["gamma"]).max())
    print("gamma(step 1e-5) - gamma(step 2e-5): %.3e" % worst)
    assert worst < 1e-9


def test_the_kkt_solution_satisfies_its_equations(solved):
    for s, i, nu, mask, r, tau in solved:
        rows = PR.rows_of(mask)
        Js = r["Jc"][rows]
        r1 = r["M"] @ r["acc"] + r["h"] - np.concatenate([np.zeros(6), tau]) - Js.T @ r["f"][rows]
        r2 = Js @ r["acc"] + r["gamma"][rows]
        scale = np.abs(r["M"]).max() * np.abs(r["acc"]).max() + np.abs(r["h"]).max() + np.abs(tau).max() + np.abs(Js).max() * np.abs(r["f"]).max()
        assert max(np.abs(r1).max(), np.abs(r2).max()) < 1e-13 * scale
        off = [k for k in range(12) if k not in rows]
        assert (r["f"][off] == 0.0).all()


def test_held_feet_do_not_accelerate_in_the_world(solved):
    """The gamma formula of include/qlamd.h, confirmed without using it: along the solved motion the world acceleration of the held
    feet, by central differences of their world velocity, goes to zero as eps^2 (a hundredfold from eps = 1e-4 to 1e-5), while a
    foot that is not held accelerates."""
    err = {1e-4: 0.0, 1e-5: 0.0}
    free = np.inf
    scale = 0.0
    for s, i, nu, mask, r, _ in solved:
        held = [l for l in range(4) if (mask >> l) & 1]
        loose = [l for l in range(4) if not (mask >> l) & 1]
        scale = max(scale, np.abs(r["acc"]).max())
        for eps in err:
            a = PR.foot_world_acceleration(s["q"][i], s["base_quat"][i], nu, r["acc"], eps)
            err[eps] = max(err[eps], np.abs(a[held]).max())
            if loose and eps == 1e-5:
                free = min(free, np.abs(a[loose]).max())
    print("world acceleration of the held feet: %.3e at eps 1e-4, %.3e at eps 1e-5; of the loose feet: >= %.3e" % (err[1e-4], err[1e-5], free))
    assert 90.0 < err[1e-4] / err[1e-5] < 110.0
    assert err[1e-5] < 1e-6 * max(1.0, scale)  # below the parity bar of the GPU tests
    assert free > 1e-2


def test_the_update_rule(oracle):
    """The restated step on cases with a known answer: a pure spin about the base z axis for one second in one step turns the base
    by exactly that angle (the exponential map is exact, not first order), and a free translation moves it along R v."""
    quat = np.array([np.cos(0.3), 0.0, np.sin(0.3), 0.0])
    z = np.zeros(12)
    n = PR.update(z, z, np.array([1.0, 2.0, 3.0]), quat, oracle.quat_to_matrix(quat) @ np.array([0.5, 0.0, 0.0]), np.array([0.0, 0.0, 2.0]),
                  np.zeros(18), 1.0)
    want = PR.quat_mul(quat, np.array([np.cos(1.0), 0.0, 0.0, np.sin(1.0)]))
    assert np.abs(n["base_quat"] - want).max() < 1e-15 and abs(np.linalg.norm(n["base_quat"]) - 1.0) < 1e-15
    assert np.abs(n["base_pos"] - (np.array([1.0, 2.0, 3.0]) + oracle.quat_to_matrix(quat) @ np.array([0.5, 0.0, 0.0]))).max() < 1e-15
    assert np.abs(n["base_linvel"] - oracle.quat_to_matrix(want) @ np.array([0.5, 0.0, 0.0])).max() < 1e-15
    # semi-implicit: the position moves with the NEW velocity
    acc = np.zeros(18); acc[6] = 4.0; acc[0] = 2.0
    n = PR.update(z, z, np.zeros(3), np.array([1.0, 0.0, 0.0, 0.0]), np.zeros(3), np.zeros(3), acc, 0.5)
    assert n["qd"][0] == 2.0 and n["q"][0] == 1.0 and n["base_linvel"][0] == 1.0 and n["base_pos"][0] == 0.5
    # small and large rotation vectors meet
    for t in (1e-9, 1e-8, 1.1e-8):
        e = PR.quat_exp(np.array([t, 0.0, 0.0]))
        assert abs(e[0] - np.cos(0.5 * t)) < 1e-16 and abs(e[1] - np.sin(0.5 * t)) < 1e-24


def test_the_library_exports_the_entry():
    from quadruped_locomotion_amd import build, capi
    lib = build.build()
    names = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    assert re.search(r" T qlamd_wholebody_forward_dynamics_batch$", names, re.M)
    assert "qlamd_wholebody_forward_dynamics_batch" in capi.EXPORTS
    assert "plant_kernel.hip" in build.SOURCE_NAMES
    assert C.sizeof(capi.PlantNext) == 48


def test_the_header_defines_the_feature_test_macro(tmp_path):
    src = tmp_path / "plant.c"
    src.write_text('#include <stddef.h>\n#include "qlamd.h"\n'
                   "#if !defined(QLAMD_HAS_PLANT_STEP) || QLAMD_HAS_PLANT_STEP != 1\n#error no plant step\n#endif\n"
                   "typedef int (*plant_fn)(qlamd_context *, const qlamd_wholebody_batch *, const double *, const double *, const double *,\n"
                   "                        double, double, int64_t, double *, double *, const qlamd_plant_next *, int32_t *, int, void *);\n"
                   "plant_fn entry = qlamd_wholebody_forward_dynamics_batch;\n"
                   "_Static_assert(sizeof(qlamd_plant_next) == 6 * sizeof(double *), \"six arrays\");\n"
                   "_Static_assert(offsetof(qlamd_plant_next, base_position) == 2 * sizeof(double *), \"order\");\n")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(src),
                           "-o", str(tmp_path / "plant.o")])


def test_the_cpp_wrapper_compiles_against_the_header(tmp_path):
    """host/qlamd/plant.hpp needs qlamd.h only: a caller of both its functions compiles with every warning an error."""
    src = tmp_path / "plant.cpp"
    src.write_text('#include "qlamd/plant.hpp"\n'
                   "int run(qlamd_context *ctx) {\n"
                   "  qlamd::host::PlantState s(3);\n  std::vector<double> tau(36), acc(54), f(36);\n  std::vector<int32_t> st(3);\n"
                   "  if (s.size() != 3 || s.base_orientation[4] != 1.0) return -1;\n"
                   "  int rc = qlamd::host::forward_dynamics(ctx, s, tau.data(), 9.81, acc.data(), f.data(), st.data());\n"
                   "  return rc != QLAMD_OK ? rc : qlamd::host::step(ctx, s, tau.data(), 9.81, 0.0025, st.data(), f.data());\n}\n")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "quadruped_locomotion_amd", "host"), "-c", str(src), "-o", str(tmp_path / "plant.o")])


def test_registers_and_scratch_are_what_design_states(tmp_path):
    """DESIGN.md 4.6c names the new kernel's registers, scratch, scratch accesses inside a loop and LDS; the figures are read from the
    device assembly compiled with the build's flags."""
    from tools import kernel_isa
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    m = re.search(r"`plant_step_kernel`: (\d+) VGPR, (\d+) AGPR, (\d+) B scratch, (\d+) scratch accesses inside a loop, (\d+) B LDS", text)
    assert m, "DESIGN.md 4.6c does not state the kernel's resources"
    stated = [int(x) for x in m.groups()]
    path = kernel_isa.assemble("plant_kernel.hip", out=str(tmp_path / "plant_kernel.s"))
    md, code = kernel_isa.meta(path), kernel_isa.kernels(path)
    names = [k for k in md if "plant_step_kernel" in k]
    assert len(names) == 1
    name = names[0]
    in_loop, loop_scratch = False, 0
    for line in code[name]:
        if line.startswith(".LBB"):
            in_loop = "in Loop" in line
        loop_scratch += in_loop and "scratch_" in line.split(";")[0]
    lds = int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", open(path).read()).group(1))
    got = [md[name]["vgpr"], md[name].get("agpr", 0), md[name].get("scratch", 0), loop_scratch, lds]
    assert got == stated, (got, stated)
    assert md[name]["vgpr"] + md[name].get("agpr", 0) <= 256  # two wavefronts per SIMD
