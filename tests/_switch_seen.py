"""The last node of every child that tests/test_gpu_switches.py starts (the file name keeps it out of a plain collection).
It prints what the parent reads back: the library's record of the EVS_* switches this process read, one SWITCH_SEEN line per
name, and the headroom every _accuracy.check of this process left, one HEADROOM line per kernel."""
import pytest

pytestmark = pytest.mark.gpu


def test_print_the_switches_seen():
    import evstore_dlrm_amd as E
    import _accuracy as acc
    print()     # (under -q -s the progress dots share the line)
    for name, was_set in E._lib.env_switches_seen().items():
        print("SWITCH_SEEN %s=%d" % (name, was_set))
    for k, (w, m, n) in sorted(acc.STATS.items()):
        print("HEADROOM\t%s\t%.4f\t%.4f\t%d" % (k, w, m, n))
