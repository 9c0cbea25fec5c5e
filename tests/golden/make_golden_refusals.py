#!/usr/bin/env python3
"""Record code and full text of the refusals of a table of cases -- tests/_batched_refusal_cases.py (the default) into
tests/golden/batched_refusals.json, tests/_fed_refusal_cases.py into tests/golden/fed_refusals.json.  Needs a GPU and the built
library.  A record pins the wording across refactors of the host orchestrators, so it is made from the commit BEFORE such a change
and not regenerated after it:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_refusals.py [_fed_refusal_cases [out.json]]
"""
import importlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]


def main():
    import evstore_dlrm_amd as E
    module = sys.argv[1] if len(sys.argv) > 1 else "_batched_refusal_cases"
    RC = importlib.import_module(module)
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(HERE, module.strip("_").replace("_refusal_cases", "_refusals") + ".json")
    record = []
    for name, build in RC.CASES:
        call, _after = build(E)
        code, text = RC.refusal(E, call)
        print("%-60s %3d  %s" % (name, code, text), flush=True)
        record.append({"case": name, "code": code, "text": text})
    with open(out, "w") as f:
        json.dump(record, f, indent=1)
        f.write("\n")
    print("%d refusals -> %s" % (len(record), out))


if __name__ == "__main__":
    main()
