"""Child of tests/test_yolo_gpu.py's kernel-trace test, run under rocprofv3 in a process of its own: the sweep of tests/yolo_sweep.py, which
launches every instantiation of libfeather_yolo.so once and compares with the restatement as it goes.  It prints the routes fhip_yolo_route
named, in launch order, for the parent to hold against the trace."""
import side_contract
import yolo_sweep as SW


def main():
    lib = side_contract.library("yolo")
    seen = []
    SW.sweep(lib, seen.append)
    for name in seen:
        print("route " + name)
    print(f"{len(seen)} launches of {len(set(seen))} routes")
    print("child ok")


if __name__ == "__main__":
    main()
