"""Child process of test_knob_routes (tests/test_attention_exact_gpu.py): started with one set of the CRG_ATTN_* developer knobs in its
environment (attention_entry reads them once per process), runs the exact attention cases named on its command line - the cases that
these knobs send to another kernel - and asserts what the parent test asserts: tests/_attention_exact_cases.py::run_and_check.  Prints
ONE JSON line {case id: "ok" or the failure}.  Not collected by pytest (leading underscore)."""
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from cremage_amd import ops  # noqa: E402
from tests import _attention_exact_cases as A  # noqa: E402


def main(ids):
    dev = torch.device("cuda:0")
    out = {}
    for cid in ids:
        case = A.BY_ID[cid]
        assert case.knobs and all(os.environ.get(k) == v for k, v in case.knobs), (cid, "started without the knobs of this case")
        try:
            A.run_and_check(case, ops, ops.HALF, dev)  # the library's half type (CRG_HALF is inherited from the parent)
            out[cid] = "ok"
        except AssertionError as e:
            out[cid] = str(e)[:600]
    print("ATTN_KNOB_RESULT " + json.dumps(out))


if __name__ == "__main__":
    with torch.no_grad():
        main(sys.argv[1:])
