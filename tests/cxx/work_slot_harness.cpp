// tests/cxx/work_slot_harness.cpp -- plade::WorkSlot / work_in (plade_amd/csrc/work_slot.h) with a counting type, no GPU: built with
// the address and undefined-behaviour sanitizers by tests/test_work_slot_host.py.  Prints one "ok <check>" line per check; the first
// check that does not hold prints "FAIL <check>" and ends the program with status 1.
#include "work_slot.h"
#include <cstdio>
#include <cstdlib>

namespace {

int made = 0, gone = 0;
struct Counted {
    int value = 7;
    Counted() { ++made; }
    ~Counted() { ++gone; }
};
struct Other {   // a second type, with its own deleter
    static int gone;
    double d[3] = {1.0, 2.0, 3.0};
    ~Other() { ++gone; }
};
int Other::gone = 0;

void check(bool ok, const char *what) {
    if (!ok) { printf("FAIL %s\n", what); exit(1); }
    printf("ok %s\n", what);
}

}  // namespace

int main() {
    using plade::WorkSlot;
    using plade::work_in;
    {
        WorkSlot s;
        check(made == 0 && s.p == nullptr, "a new slot holds nothing");
        Counted &a = work_in<Counted>(s);
        check(made == 1 && gone == 0 && a.value == 7, "first use creates");
        a.value = 11;
        Counted &b = work_in<Counted>(s);
        check(&a == &b && made == 1 && b.value == 11, "later uses return the same object");
        s.reset();
        check(made == 1 && gone == 1 && s.p == nullptr, "reset deletes once");
        s.reset();
        check(gone == 1, "reset is idempotent");
    }
    check(made == 1 && gone == 1, "destruction after reset deletes nothing");
    {
        WorkSlot s;
        work_in<Counted>(s);
        s.reset();
        Counted &c = work_in<Counted>(s);
        check(made == 3 && gone == 2 && c.value == 7, "a reset slot creates afresh");
    }
    check(made == 3 && gone == 3, "destruction deletes what reset did not");
    {
        WorkSlot icp, gicp;   // two slots of one type, as the two refinements
        Counted &a = work_in<Counted>(icp), &b = work_in<Counted>(gicp);
        a.value = 1; b.value = 2;
        check(&a != &b && made == 5, "two slots of one type hold two objects");
        check(work_in<Counted>(icp).value == 1 && work_in<Counted>(gicp).value == 2, "each slot keeps its own");
        icp.reset();
        check(gone == 4 && gicp.p == &b && b.value == 2, "resetting one leaves the other");
    }
    check(made == 5 && gone == 5, "both are gone at the end");
    {
        WorkSlot unused;
    }
    check(made == 5 && gone == 5, "a slot that was never used destroys cleanly");
    {
        WorkSlot s, t;
        work_in<Other>(s);
        work_in<Counted>(t);
    }
    check(Other::gone == 1 && made == 6 && gone == 6, "each type is deleted by its own deleter");
    return 0;
}
