"""CPU-only checks of bench.py's command line: a plain run is the headline alone, the legs that take runs of their own wait
for --full."""
import bench


def test_full_is_off_by_default():
    assert not bench.parse([]).full
    assert not bench.parse(["--gpus", "1", "--steps", "3", "--warmup", "1"]).full
    assert bench.parse(["--full"]).full
