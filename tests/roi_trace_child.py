"""Child of tests/test_roi_gpu.py's kernel-trace test, run under rocprofv3 in a process of its own: the sweep of tests/roi_sweep.py, which
launches every instantiation of libfeather_roi.so once and compares with the restatement as it goes.  It prints the routes fhip_roi_route
named, in launch order, for the parent to hold against the trace."""
import roi_sweep as SW
import side_contract


def main():
    lib = side_contract.library("roi")
    seen = []
    SW.sweep(lib, seen.append)
    for name in seen:
        print("route " + name)
    print(f"{len(seen)} launches of {len(set(seen))} routes")
    print("child ok")


if __name__ == "__main__":
    main()
