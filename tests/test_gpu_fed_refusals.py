"""Every refusal of the fed begin / finish / abort calls, and of the other calls on a fed cache, keeps its return code and its full
evs_last_error() text: the table of tests/_fed_refusal_cases.py replayed against tests/golden/fed_refusals.json (recorded by
tests/golden/make_golden_refusals.py from the commit before the two begins and the two finishes were put on one frame, never
regenerated).  A refusal that leaves a call open leaves it to the right finish, and the call after that is a twin cache's."""
import json
import os

import pytest
import torch

import _fed_refusal_cases as RC

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fed_refusals.json")) as _f:
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
