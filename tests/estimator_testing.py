"""What the tests of the batched estimators (test_pose_refine,
test_generalized_pose, test_relative_pose, test_triangulation) and their case
modules share: quaternions for the synthetic scenes, ulp perturbations of a
problem, the LM traces as comparable sequences, and the C++ test programs of
tests/cpp."""
import os
import subprocess

import numpy as np

CPP = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp")


def quat(axis_angle):
    a = np.linalg.norm(axis_angle)
    if a == 0:
        return np.array([1.0, 0, 0, 0])
    return np.concatenate([[np.cos(a / 2)], np.sin(a / 2) * np.asarray(axis_angle) / a])


def qmul(z, w):
    return np.array([z[0] * w[0] - z[1:] @ w[1:], *(z[0] * w[1:] + w[0] * z[1:] + np.cross(z[1:], w[1:]))])


def ulp_perturbed(problem, rng, names):
    """The problem with every coordinate of its arrays `names` moved by -1, 0
    or +1 ulp."""
    b = problem.copy()
    for name in names:
        a = getattr(b, name)
        s = rng.choice([-1, 0, 1], a.shape).astype(float)
        a[:] = np.where(s == 0, a, np.nextafter(a, a + s))
    return b


def ulp_solves(problem, solve, names):
    """solve(perturbed problem) of three ulp perturbations of the inputs, one
    after the other (a caller may stop early)."""
    rng = np.random.default_rng(7)
    for _ in range(3):
        yield solve(ulp_perturbed(problem, rng, names))


def same_stop(a, b):
    """The step counts and the stop of two summaries or reference results:
    whether a solver's stop is decided by rounding (tests/test_lm_semantics.py)
    shows in them under ulp_solves."""
    return (a.num_successful_steps, a.num_unsuccessful_steps, a.termination_type) == (
        b.num_successful_steps, b.num_unsuccessful_steps, b.termination_type)


def hexes(xs):
    return " ".join(float(x).hex() for x in np.asarray(xs, np.float64).reshape(-1))


def oracle_sequence(trace):
    """(valid, successful, ended) per iteration of the oracle trace."""
    return [(int(v), int(s), int(e)) for v, s, _, e in trace]


def gpu_sequence(row):
    """The same of one row of the device's LM trace (mi_ba_pose_refine_set_trace)."""
    return [(int(b) & 1, (int(b) >> 1) & 1, (int(b) >> 2) & 1) for b in row if b != 0xFF]


def make(target):
    """Builds one target of tests/cpp/Makefile; returns its path."""
    subprocess.run(["make", "-C", CPP, target], check=True, capture_output=True)
    return os.path.join(CPP, target)


def run_program(target, *args, timeout=300):
    out = subprocess.run([make(target), *args], capture_output=True, text=True, timeout=timeout)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "0 failure(s)" in out.stdout
    return out.stdout
