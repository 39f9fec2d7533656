"""Child of tests/test_rnn_gpu.py's kernel-trace test, run under rocprofv3 in a process of its own: the sweep of tests/rnn_sweep.py, which
launches every instantiation of libfeather_rnn.so and compares with the restatement as it goes.  It prints the routes fhip_rnn_route named,
in launch order (T lines for a call on the step route), for the parent to hold against the trace."""
import rnn_sweep as SW
import side_contract


def main():
    lib = side_contract.library("rnn")
    seen = []
    SW.sweep(lib, seen.append)
    for name in seen:
        print("route " + name)
    print(f"{len(seen)} launches of {len(set(seen))} routes")
    print("child ok")


if __name__ == "__main__":
    main()
