"""The dense Levenberg-Marquardt of the CPU references, once: Ceres 2.1's
TrustRegionMinimizer with LevenbergMarquardtStrategy (Jacobi scaling fixed at
iteration 0, the diagonal clipped to [1e-6, 1e32], the radius rules of
rig_reference.RigProblem.solve) plus the gradient, parameter and function
tolerance stops and the limit on consecutive invalid steps.

generalized_pose_reference.Problem and relative_pose_reference.Problem are the
problems it runs on.  A problem has
    jacobian()       -> (loss-corrected r, tangent J, cost) at its state
    plus(delta)      -> the candidate state, a tuple
    cost(*state)     -> the cost at a candidate
    ambient(*state)  -> the concatenated ambient vector (no arguments: of its
                        own state), for the gradient and parameter tests
    accept(*state)   -> takes the candidate as its state
"""
from collections import namedtuple

import numpy as np

CONVERGENCE, NO_CONVERGENCE, FAILURE = 0, 1, 2

# trace: (valid, successful, ended) per iteration
Solve = namedtuple("Solve", "initial_cost final_cost num_successful_steps num_unsuccessful_steps termination_type trace")


# rig_reference.RigProblem.solve stays its own loop: no convergence tests, 10 invalid steps, a reused damping
# diagonal and another trace; it would add switches here, not remove code.
def minimize(p, gradient_tolerance, max_num_iterations, function_tolerance=1e-6, parameter_tolerance=1e-8,
             max_num_consecutive_invalid_steps=5, initial_trust_region_radius=1e4, min_relative_decrease=1e-3):
    """Minimizes p from its state (which must have residuals); p is left at
    the last accepted state, also after FAILURE."""
    r, J, x_cost = p.jacobian()
    initial = x_cost
    if not np.isfinite(x_cost):
        return Solve(initial, x_cost, 0, 0, FAILURE, [])
    scale = 1.0 / (1.0 + np.sqrt((J * J).sum(0)))  # Jacobi scaling, fixed at iteration 0
    radius, decrease_factor = initial_trust_region_radius, 2.0
    ns = nu = invalid = iteration = 0
    last_successful, trace, term = True, [], NO_CONVERGENCE
    while True:
        if iteration >= max_num_iterations:
            term = NO_CONVERGENCE
            break
        if last_successful:
            g = J.T @ r
            if np.abs(p.ambient() - p.ambient(*p.plus(-g))).max() <= gradient_tolerance:
                term = CONVERGENCE
                break
        if radius <= 1e-32:
            term = CONVERGENCE
            break
        iteration += 1
        Js = J * scale
        diag = np.clip((Js * Js).sum(0), 1e-6, 1e32)
        A = Js.T @ Js + np.diag(diag / radius)
        ok = True
        try:
            L = np.linalg.cholesky(A)
            y = np.linalg.solve(L.T, np.linalg.solve(L, -(Js.T @ r)))
        except np.linalg.LinAlgError:
            ok = False
        model_change = 0.0
        if ok:
            delta = y * scale
            mr = J @ delta
            model_change = -mr @ (r + mr / 2)
            ok = bool(np.isfinite(model_change) and model_change > 0)
        if not ok:
            invalid += 1
            nu += 1
            last_successful = False
            radius /= decrease_factor
            decrease_factor *= 2
            end = invalid > max_num_consecutive_invalid_steps
            trace.append((0, 0, int(end)))
            if end:
                term = FAILURE
                break
            continue
        invalid = 0
        candidate = p.plus(delta)
        cand_cost = p.cost(*candidate)
        x_amb = p.ambient()
        step_norm = np.linalg.norm(x_amb - p.ambient(*candidate))
        cost_change = x_cost - cand_cost
        if step_norm <= parameter_tolerance * (np.linalg.norm(x_amb) + parameter_tolerance) or \
                abs(cost_change) <= function_tolerance * x_cost:
            nu += 1
            term = CONVERGENCE
            trace.append((1, 0, 1))
            break
        rel = cost_change / model_change
        if np.isfinite(cand_cost) and rel > min_relative_decrease:
            ns += 1
            last_successful = True
            x_cost = cand_cost
            p.accept(*candidate)
            radius = min(1e16, radius / max(1.0 / 3.0, 1.0 - (2.0 * rel - 1.0) ** 3))
            decrease_factor = 2.0
            r, J, _ = p.jacobian()
            trace.append((1, 1, 0))
        else:
            nu += 1
            last_successful = False
            radius /= decrease_factor
            decrease_factor *= 2
            trace.append((1, 0, 0))
    return Solve(initial, x_cost, ns, nu, term, trace)
