"""Every evaluator of the closure plan (model._closure_plan) through the shared graph runner (_optim.GraphRunner) once:
a short fit with the closure replayed from its HIP graph against the same fit run eagerly."""
import numpy as np
import pytest
import torch
from torch.nn.utils.parametrize import register_parametrization

import model_cases as mc
from conftest import rel_err

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

# (evaluator, model, filters K, constraint, distance_fun, rows held by a FixedFilters stage)
CASES = [
    ("single_node", "smsqfa", 2, "sphere", None, 0),
    ("single_node", "smsqfa", 2, "none", None, 0),
    ("single_node", "smsqfa", 2, "orthogonal", None, 0),
    ("single_node", "sqfa", 2, "sphere", None, 0),
    ("chain", "smsqfa", 2, "sphere", None, 1),
    ("chain", "sqfa", 3, "sphere", None, 1),
    ("gauss", "sqfa", 2, "sphere", "bhattacharyya", 0),
    ("log_euclidean", "smsqfa", 2, "sphere", "log_euclidean", 0),
]


@pytest.fixture(scope="module")
def statistics():
    return mc.c2_statistics(C=3, D=8)


# float64: the bounds of test_gpu_model.test_graph_captured_closure_matches_eager; float32: test_gpu_model's float32
# closure bounds (1e-5 on the loss, 2e-5 on values derived from it)
@pytest.mark.parametrize("dtype,tol_loss,tol_filters", [(torch.float64, 1e-12, 1e-10), (torch.float32, 1e-5, 2e-5)])
@pytest.mark.parametrize("evaluator,model_name,K,constraint,fn,fixed", CASES)
def test_every_evaluator_replays_what_it_evaluates_eagerly(evaluator, model_name, K, constraint, fn, fixed, dtype,
                                                           tol_loss, tol_filters, statistics, monkeypatch):
    import sqfa_amd._optim as opt
    from sqfa_amd import distances
    from sqfa_amd.constraints import FixedFilters
    stats = {k: v.to(dtype).to(DEV) for k, v in statistics.items()}
    data = stats if model_name == "sqfa" else stats["covariances"] + stats["means"][:, :, None] * stats["means"][:, None, :]
    monkeypatch.setattr(opt, "GRAPH_WARMUP_CLOSURES", 1)
    replays = [0]
    original_replay = torch.cuda.CUDAGraph.replay

    def counting_replay(self):
        replays[0] += 1
        return original_replay(self)

    monkeypatch.setattr(torch.cuda.CUDAGraph, "replay", counting_replay)
    runs = {}
    for use_graph in (False, True):
        monkeypatch.setattr(opt, "GRAPH_CLOSURE", use_graph)
        torch.manual_seed(3)
        model = mc.make_model(model_name, 8, K, 0.01, constraint, dtype, DEV)
        if constraint == "orthogonal":   # torch registers a transposed view as `base`; the native map takes a contiguous one
            mc.set_orthogonal_base(model, model.parametrizations.filters[0].base.contiguous())
        if fn is not None:
            model.distance_fun = getattr(distances, fn)
        if fixed:
            register_parametrization(model, "filters", FixedFilters(n_row_fixed=fixed))
        assert model._closure_plan(model._prepare_statistics(data)).evaluator == evaluator
        loss, _ = model.fit(data_statistics=data, max_epochs=4, show_progress=False, return_loss=True)
        runs[use_graph] = (loss.numpy(), model.filters.detach().cpu().numpy())
        if not use_graph:
            assert replays[0] == 0
    assert replays[0] >= 1, "the graph path was not taken"
    assert np.abs(runs[True][0] - runs[False][0]).max() < tol_loss
    assert rel_err(runs[True][1], runs[False][1]) < tol_filters
