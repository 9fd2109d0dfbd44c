"""CPU test: bench.py's command line.  A plain run is the lean one -- every leg that takes runs of its own waits for
--full -- and the flags that select among those legs keep their names and defaults."""
import bench


def test_full_is_an_option_that_is_off_by_default():
    ap = bench.make_parser()
    plain = ap.parse_args(["--gpus", "1", "--steps", "20", "--warmup", "5"])
    assert plain.full is False
    assert (plain.gpus, plain.steps, plain.warmup) == (1, 20, 5)
    assert plain.dump_outputs is None and plain.graph is False and plain.io == "f32"
    full = ap.parse_args(["--gpus", "1", "--steps", "20", "--warmup", "5", "--full"])
    assert full.full is True
    assert {k: v for k, v in vars(full).items() if k != "full"} == {k: v for k, v in vars(plain).items() if k != "full"}


def test_the_flags_that_trim_a_full_run_are_still_there():
    a = bench.make_parser().parse_args(["--full", "--no-cpu-baseline", "--no-extra-configs", "--dump-outputs", "d"])
    assert a.full and a.no_cpu_baseline and a.no_extra_configs and a.dump_outputs == "d"
    d = bench.make_parser().parse_args([])
    assert (d.gpus, d.steps, d.warmup, d.batch, d.spinup_ms) == (1, 50, 10, bench.B_PER_GPU, 150.0)
    assert not d.no_cpu_baseline and not d.no_extra_configs
