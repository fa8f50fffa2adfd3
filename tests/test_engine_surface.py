"""CPU test of the fused engine's surface: FusedMLP is assembled from vbnn_amd/engine.py (construction, the step, the exchange),
predictive.py and pruning.py. Whatever moves between those modules, every name a host, a tool or a test reaches through
FusedMLP or imports from vbnn_amd.engine stays, and the main entry points keep their parameters."""
import inspect

# every non-dunder attribute of the class, as of the last commit that held it in one module
ATTRIBUTES = [
    "_alloc_batch", "_build", "_build_dw_args", "_build_dx_args", "_build_fwd_args", "_compress", "_dw_args", "_dx_args", "_early",
    "_fwd_args", "_generic_head", "_held_ptrs", "_lrt", "_need_gathered_parameters", "_on_stream", "_predict_buffers",
    "_predict_forward", "_predict_forward_sparse", "_predict_stacked", "_predict_weights", "_predict_wn_sample", "_probed",
    "_probed_part", "_prune_descs", "_prune_mask", "_reduce", "_refuse_held", "_scatter", "_sparse_buffers", "_unit_descs",
    "_update_sharded", "_use_head_slots", "buckets", "calc_lc", "capture_step", "check_exchange", "clamp_to_map", "comm_backend",
    "compact", "exchange", "finish", "gather_parameters", "held", "held_mask", "hold_pruned", "init_parameters", "join",
    "loss_and_accuracy", "predict", "predict_regression", "prepare", "probe", "prune", "prune_curve", "prune_curve_sparse",
    "prune_units", "prune_units_curve", "pruned", "release_pruned", "resetGradients", "run", "run_draws", "sample", "skip_exchange",
    "snr", "synthetic_targets", "test", "time_buckets", "unit_snr", "update", "use_pruned"]
RESULT_CLASSES = ["PredictResult", "RegressionPredictResult", "PruneResult", "SparsePruneResult", "UnitPruneResult"]
SIGNATURES = {
    "predict": ["self", "inputs", "S", "targets", "map", "row0"],
    "predict_regression": ["self", "inputs", "S", "targets", "noise_var", "map", "row0", "keep_draws"],
    "prune": ["self", "fraction", "threshold", "scope"],
    "prune_units": ["self", "fraction", "threshold", "scope", "multiple"],
    "compact": ["self", "result", "opt_overrides"],
    "hold_pruned": ["self", "result"],
    "update": ["self", "opt", "log"],
    "run": ["self", "inputs", "targets", "row0", "backward", "last_draw"],
}


def test_nothing_disappears_from_the_engine():
    from vbnn_amd import engine
    assert len(ATTRIBUTES) == 71 and ATTRIBUTES == sorted(ATTRIBUTES) and ATTRIBUTES[0] == "_alloc_batch" and ATTRIBUTES[-1] == "use_pruned"
    have = set(dir(engine.FusedMLP))
    assert not [n for n in ATTRIBUTES if n not in have], [n for n in ATTRIBUTES if n not in have]
    for name in RESULT_CLASSES:
        assert inspect.isclass(getattr(engine, name, None)), name
    for name, params in SIGNATURES.items():
        assert list(inspect.signature(getattr(engine.FusedMLP, name)).parameters) == params, name
