"""Child process of tests/test_gpu_restart.py: MQC_HIP_HBM_BUDGET_GB and MQC_HIP_SCF_WIDE_MAX are read once per process,
so the chunked route and the 256-thread kernels run the mixed restart batch in a process of their own:
`python -m tests.restart_child OUT.json`, with the route's environment set by the parent.  Test infrastructure."""
import json
import sys

from tests import test_gpu_restart as t


def main(out):
    rec = t.mixed_batch_restart()
    with open(out, "w") as f:
        json.dump({"e": [float(v) for v in rec["e_total"]], "it": [int(v) for v in rec["iterations"]],
                   "err": [int(v) for v in rec["has_error"]]}, f)
    print(json.dumps({"file": out, "fragments": len(rec)}))


if __name__ == "__main__":
    main(sys.argv[1])
