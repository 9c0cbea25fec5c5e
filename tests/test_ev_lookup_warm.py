"""Warm start of the cache manager behind ev_lookup (evs_manager_export / evs_manager_load through
cache_algo/cpp_socket_client.save_state / load_state), host engine: N lookups in one process, save_state, a SECOND process
that loads the file and continues -- the concatenated rows and the perfect-hit counter are those of one process that ran all
lookups.  The manager is a process-wide singleton, hence the children.  No GPU involved."""
import numpy as np
import pytest

import _exact_warm as W


@pytest.mark.parametrize("layers", [1, 2])
def test_a_second_process_loads_and_continues(tmp_path, layers):
    W.check_two_processes(tmp_path, layers)


def test_three_layers_are_refused(tmp_path):
    W.write_tables(tmp_path, 10)
    (tmp_path / "altkeys").mkdir()
    for k, w in enumerate(W.tables()):
        ((np.arange(len(w)) * 100 + (k + 1)).astype(">u4")).tofile(tmp_path / "altkeys" / ("ev-table-%d.bin" % (k + 1)))
    state = np.zeros(20, np.int64)
    state[:6] = [2, 0, 96, 26, 36, 8]
    with open(tmp_path / "given.npz", "wb") as f:          # a well-formed (empty) state: refused for the layers, not for its content
        np.savez(f, entries1=np.zeros((0, 3), np.int64), state1=state)
    r = W.manager_child(tmp_path, 3, 0, 10, tmp_path / "given.npz", tmp_path / "state.npz", tmp_path / "x.npy",
                        env_extra={"EVS_ALTKEY_DIR": str(tmp_path / "altkeys"), "EVS_SIZE_PROPORTION": "40-40-20"})
    assert r["refused"] == -1 and r["refused_load"] == -1   # EVS_EINVAL both ways: the alt-key tier has no export
    assert r["served"]                                  # ... and the manager serves all the same
