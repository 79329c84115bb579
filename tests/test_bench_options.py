"""bench.py --full: a plain run measures nothing beside its timed steps; --full measures what the configuration has, and the
--no-* options take parts of it out again."""
import bench

PLAIN_ARGS = [[], ['--workload', 'C5', '--scaling', 'strong'], ['--small', '--rehearse-legs'], ['--steps', '20', '--warmup', '5'],
              ['--no-legs', '--no-extras', '--no-single-solve', '--no-cpu-baseline']]


def test_plain_run_measures_only_its_steps():
    assert bench.parse_args([]).full is False
    for argv in PLAIN_ARGS:
        for world in (1, 2, 8):
            ex = bench.extras(bench.parse_args(argv), world)
            assert not any(ex.values()), (argv, world, ex)


def test_full_run_measures_every_extra_of_the_headline_configuration():
    ex = bench.extras(bench.parse_args(['--full']), 1)
    assert all(v for k, v in ex.items() if k != 'strong') and not ex['strong'], ex
    ex = bench.extras(bench.parse_args(['--full']), 8)
    assert ex['kernel_profile'] and ex['strong'], ex
    assert not any(v for k, v in ex.items() if k not in ('kernel_profile', 'strong')), ex


def test_no_options_take_parts_of_full_out():
    ex = bench.extras(bench.parse_args(['--full', '--no-legs', '--no-extras', '--no-single-solve', '--no-cpu-baseline']), 1)
    assert ex == dict.fromkeys(ex, False) | {'kernel_profile': True}, ex
    ex = bench.extras(bench.parse_args(['--full', '--no-cpu-baseline']), 1)
    assert not ex['cpu_baseline'] and ex['legs'] and ex['single_solve'], ex
    assert not bench.extras(bench.parse_args(['--full', '--workload', 'C5']), 1)['legs']
