"""Every refusal the batched cache calls make before anything is launched keeps its return code and its full evs_last_error()
text: the table of tests/_batched_refusal_cases.py replayed against tests/golden/batched_refusals.json (recorded by
tests/golden/make_golden_refusals.py from the commit before the host orchestrators were folded together, never regenerated).
After a refusal that saw or resolved a batch policy the cache still takes the opposite one and serves."""
import json
import os

import pytest
import torch

import _batched_refusal_cases as RC

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "batched_refusals.json")) as _f:
    GOLDEN = {r["case"]: r for r in json.load(_f)}


@pytest.fixture(scope="module")
def E():
    import evstore_dlrm_amd as E
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    E._lib.lib()
    return E


def test_the_record_covers_the_table():
    assert sorted(GOLDEN) == sorted(name for name, _b in RC.CASES)


@pytest.mark.parametrize("name,build", RC.CASES, ids=[name for name, _b in RC.CASES])
def test_refusal_keeps_its_code_and_text(E, name, build):
    call, after = build(E)
    code, text = RC.refusal(E, call)
    print(name, code, text)
    assert (code, text) == (GOLDEN[name]["code"], GOLDEN[name]["text"])
    if after:
        after()
    assert E._lib.lib().evs_check_index_errors(None) == 0
