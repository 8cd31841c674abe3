"""The limits of tests/test_autograd_nodes_gpu.py are the stated ones (1e-4 in f32, 1e-2 for a single bf16 node) or three
times a figure recorded in tests/autograd_node_cases.py -- and that figure is what the measurement gives: the case's
float64 reference with a bf16 rounding at every stored tensor against the same reference without, on the CPU.  The cases
are imported from the GPU test file; nothing here touches a device or the native library."""
import autograd_node_cases as NC


def test_limits_are_the_stated_ones_or_three_times_a_recorded_measurement():
    assert NC.LIMIT == {"f32": 1e-4, "bf16": 1e-2} and NC.MEASURED_FACTOR == 3.0
    for name, c in NC.CASES.items():
        assert set(c.dtypes) <= {"f32", "bf16"} and c.dtypes, name
        assert NC.limit(name, "f32", "d x") == 1e-4, name
        if c.measured is None:
            assert NC.limit(name, "bf16", "d x") == 1e-2, name
        elif isinstance(c.measured, dict):
            assert "" in c.measured, name
            for what, m in c.measured.items():
                assert NC.limit(name, "bf16", what or "d x") == 3.0 * m, (name, what)
        else:
            assert NC.limit(name, "bf16", "d x") == 3.0 * c.measured, name


def test_recorded_measurements_are_current():
    """Within a factor of two either way: the figures depend on the last bits of float64 sums (and, where ReLU units flip,
    on single units), so another BLAS may move them a little; a case whose shapes, seeds or reference changed moves them
    by more, and then the table has to be measured again (`python tests/test_autograd_nodes_gpu.py`)."""
    import test_autograd_nodes_gpu as T
    for name, c in NC.CASES.items():
        if c.measured is None:
            continue
        now = T.measured_as_recorded(name)
        pairs = [(k, c.measured[k], now[k]) for k in c.measured] if isinstance(c.measured, dict) else [("", c.measured, now)]
        for what, recorded, err in pairs:
            assert 0.5 * recorded <= err <= 2.0 * recorded, (name, what, err, recorded)
