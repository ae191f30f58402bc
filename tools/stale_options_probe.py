"""Can tests/test_gpu_batch_options.py see a leak?  Runs its one-context case on
every host path, zero and NIC checks, first as it is (passes), then with a
HostPath.submit that hands one batch in seven the PREVIOUS call's options and
ingress -- what a stale slot or ring header would amount to.  Every mutated
run must fail its comparison; exits 1 if one survives.  Needs a GPU; run from
the repository root."""
import sys, os
sys.path.insert(0, os.getcwd()); sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import torch
from xsknf_amd import HostPath, Checksummer, ChecksummerOptions
import tests.test_gpu_batch_options as T

real = HostPath.submit
state = {"n": 0, "prev": None}
def stale(self, descs, verdicts, ingress_ifindex=0, opts=None):
    state["n"] += 1
    cur = (ingress_ifindex, opts)
    if state["n"] % 7 == 0 and state["prev"] is not None:
        ingress_ifindex, opts = state["prev"]
    state["prev"] = cur
    return real(self, descs, verdicts, ingress_ifindex, opts)

cs = Checksummer(ChecksummerOptions(action=1, csum_iterations=5), num_interfaces=7, frame_len_hint=1500)
dev = torch.device("cuda:0")
fn = T.test_one_context_batches_in_flight
bad = 0
for path in ("zerocopy", "staged", "resident"):
    for checks in ("zero", "nic"):
        state.update(n=0, prev=None)
        HostPath.submit = real
        fn(dev, cs, path, checks)                     # unmutated: passes
        HostPath.submit = stale
        try:
            fn(dev, cs, path, checks)
            print("MUTANT SURVIVED", path, checks); bad += 1
        except AssertionError as e:
            print("caught", path, checks, "::", str(e)[:200])
HostPath.submit = real
sys.exit(1 if bad else 0)
