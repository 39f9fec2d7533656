"""Child of tests/test_attn_gpu.py's kernel-trace test, run under rocprofv3 in a process of its own: the sweep of tests/attn_sweep.py, which
launches every instantiation of libfeather_attn.so once and compares with the restatement as it goes.  It prints the routes
fhip_attn_route named, in launch order, for the parent to hold against the trace."""
import attn_sweep as SW
import side_contract


def main():
    lib = side_contract.library("attn")
    seen = []
    SW.sweep(lib, seen.append)
    for name in seen:
        print("route " + name)
    print(f"{len(seen)} launches of {len(set(seen))} routes")
    print("child ok")


if __name__ == "__main__":
    main()
