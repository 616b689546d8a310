"""CPU: the two replays share the filter's segment propagator (``particle_filter._segment_propagator``) and its normals
(``particle_filter.path_normals``).

The one identity that holds exactly only then: PMMH's record replay (``particle_mcmc.replay_path_records``), fed the records of the
smoother's own draws (its start states as anchors, its noise paths, the call's key for every record), returns the smoother's paths
bit for bit.  float64 and float32, OU / Lotka-Volterra / SIR (the latter two with positive dims, so the clamp binds), the three
proposals, and the two row sets of tests/particle_smoother_reference.py: a first segment from row 0 and one with steps of its own, a
repeated row, a segment inside one Philox block of four and segments that cross blocks.  No tolerance."""
import numpy as np
import pytest
import torch

import particle_smoother_reference as sref

M, N, D = 3, 16, 5


def _key(k0, k1):
    return torch.from_numpy(np.array([k0, k1], dtype=np.uint32).view(np.int32))


@pytest.mark.parametrize("rows", [sref.BLOCK_ROWS, sref.LATE_ROWS], ids=["block", "late"])
@pytest.mark.parametrize("proposal", ["bootstrap", "bridge", "residual_bridge"])
@pytest.mark.parametrize("name", ["ou", "lv", "sir"])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_record_replay_of_the_smoothers_draws_is_the_smoothers_paths(dtype, name, proposal, rows):
    from viforsdes_amd import Observations, particle_filter, particle_smoother
    from viforsdes_amd.inference import particle_filter as pf
    from viforsdes_amd.inference.particle_mcmc import replay_path_records
    assert tuple(pf.PROPOSALS) == ("bootstrap", "bridge", "residual_bridge")
    sde, obs, like, th, x0, dt, pos = sref.case(name, M, rows=rows)
    obs = Observations(times=obs.times.to(dtype), values=obs.values.to(dtype))
    th, x0, key = th.to(dtype), x0.to(dtype), _key(0x1F83D9AB, 0x5BE0CD19)
    kw = dict(n_particles=N, initial_state=x0, positive_dims=pos, key=key, proposal=proposal)
    smoothed = particle_smoother(sde, obs, like, th, dt, n_draws=D, **kw)
    filtered = particle_filter(sde, obs, like, th, dt, return_particles=True, **kw)
    K, S, T = len(rows), x0.shape[1], rows[-1]
    lineage = smoothed.lineage.long()                                                       # [M, D, K]
    assert bool((lineage >= 0).all())
    # anchors[b, k] = particles[m, k, lineage[m, d, k]], noise_path[b, k] = m N + lineage[m, d, k], b = m D + d
    anchors = torch.gather(filtered.particles, 2, lineage.permute(0, 2, 1)[..., None].expand(M, K, D, S)).permute(0, 2, 1, 3)
    noise_path = torch.arange(M)[:, None, None] * N + lineage
    paths = replay_path_records(sde, obs, like, th.repeat_interleave(D, dim=0), x0.repeat_interleave(D, dim=0),
                                anchors.reshape(M * D, K, S), noise_path.reshape(M * D, K), key.expand(M * D, 2), float(dt), pos,
                                proposal != "bootstrap", proposal == "residual_bridge")
    assert torch.equal(paths.reshape(M, D, T + 1, S), smoothed.paths)
    assert bool(torch.isfinite(smoothed.paths).all())
