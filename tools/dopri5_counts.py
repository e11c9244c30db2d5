"""The count model of the exact mode's kernels (pure numpy, no GPU): what a wave of 64 consecutive envs pays, in RHS
evaluations, when its lanes step in lock step minute by minute (t1d_step_dopri5) and when they run free inside a launch
and wait for each other only at its end (t1d_rollout_*_dopri5).  Operation counts, not times."""
import numpy as np


def wave_costs(nfev, launch_minutes, wave=64):
    """nfev: [minutes][n] RHS evaluations of each env in each minute.  -> dict, all per env-minute:
      rhs_per_env_minute      the mean: what the arithmetic itself needs
      lockstep_wave_cost      mean over the waves of the per-minute maximum over the wave's lanes (a wave runs each minute
                              until its slowest lane is done)
      free_running_wave_cost  launches of launch_minutes minutes: mean over the waves of the maximum over the wave's lanes of
                              the lane's total in a launch, summed over the launches
    A last wave with fewer than `wave` lanes counts as a wave; a last launch may be shorter."""
    nf = np.asarray(nfev, dtype=np.float64)
    minutes, n = nf.shape
    pad = (-n) % wave
    if pad:
        nf = np.concatenate([nf, np.zeros((minutes, pad))], axis=1)
    w = nf.reshape(minutes, -1, wave)
    lock = w.max(axis=2).sum(axis=0)
    free = np.zeros(w.shape[1])
    for m0 in range(0, minutes, int(launch_minutes)):
        free += w[m0:m0 + int(launch_minutes)].sum(axis=0).max(axis=1)
    return {"rhs_per_env_minute": float(nf.sum() / (minutes * n)),
            "lockstep_wave_cost": float(lock.mean() / minutes),
            "free_running_wave_cost": float(free.mean() / minutes)}
