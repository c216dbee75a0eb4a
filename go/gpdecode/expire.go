package gpdecode

// Flow expiry (include/gpd_flow_expire.h) from Go: StreamPool.remove and the idle test of
// FlushOlderThan / FlushCloseOlderThan for the flow table, so that a capture runs without
// FlowTable.Reset.  Not compiled here (no Go toolchain); tests/test_flow_expire_gpu.py drives the
// same C entry points through ctypes on the GPU.

/*
#cgo CFLAGS: -I${SRCDIR}/../../include -I/opt/rocm/include -D__HIP_PLATFORM_AMD__
#cgo LDFLAGS: -L/opt/rocm/lib -lamdhip64
#include <hip/hip_runtime_api.h>
#include "gpd.h"
#include "gpd_flow.h"
#include "gpd_flow_expire.h"
*/
import "C"

import (
	"fmt"
	"unsafe"
)

// Remove is StreamPool.remove for the listed flow records.  Ids at or above the capacity, ids of
// empty slots and duplicates are ignored.
func (t *FlowTable) Remove(ids []uint32) error {
	if len(ids) == 0 {
		return nil
	}
	done, err := t.parser.onDevice()
	if err != nil {
		return err
	}
	defer done()
	d, err := devAlloc(4 * len(ids))
	if err != nil {
		return err
	}
	defer d.free()
	if err := toDev(d, unsafe.Pointer(&ids[0]), 4*len(ids)); err != nil {
		return err
	}
	if rc := C.gpd_flow_remove(t.ft, (*C.uint32_t)(d.p), C.uint64_t(len(ids)), nil); rc != C.GPD_OK {
		return lastError("gpd_flow_remove", rc)
	}
	if rc := C.hipDeviceSynchronize(); rc != 0 {
		return lastError("hipDeviceSynchronize", C.GPD_ERR_HIP)
	}
	return nil
}

// Expire removes every record whose last packet's sequence number is below olderThanSeq (strictly,
// as time.Before; 0 removes nothing), except those with hold[id] != 0 (hold: nil, or one byte per
// record of the table).  With pairs a record leaves only together with the record of its reversed
// key, so that both halves of a reassembly connection leave together.  It returns the removed ids,
// ascending: hand them to ConnTracker.Forget.
//
//	ids, _ := table.Expire(oldestYoungBatchSeq, hold, true)
//	_ = tracker.Forget(ids)
func (t *FlowTable) Expire(olderThanSeq uint64, hold []uint8, pairs bool) ([]uint32, error) {
	done, err := t.parser.onDevice()
	if err != nil {
		return nil, err
	}
	defer done()
	var fst C.gpd_flow_stats
	if rc := C.gpd_flow_stats_get(t.ft, &fst, nil); rc != C.GPD_OK {
		return nil, lastError("gpd_flow_stats_get", rc)
	}
	capacity := int(fst.capacity)
	var dhold *C.uint8_t
	if hold != nil {
		if len(hold) < capacity {
			return nil, fmt.Errorf("gpdecode: Expire: hold has %d bytes, the table %d records", len(hold), capacity)
		}
		d, err := devAlloc(capacity)
		if err != nil {
			return nil, err
		}
		defer d.free()
		if err := toDev(d, unsafe.Pointer(&hold[0]), capacity); err != nil {
			return nil, err
		}
		dhold = (*C.uint8_t)(d.p)
	}
	flags := C.uint32_t(0)
	if pairs {
		flags = C.GPD_FLOW_EXPIRE_PAIRS
	}
	// the sizing call, the allocation, then the removal
	var count C.uint64_t
	if rc := C.gpd_flow_expire(t.ft, C.uint64_t(olderThanSeq), dhold, flags, nil, 0, &count, nil); rc != C.GPD_OK {
		return nil, lastError("gpd_flow_expire", rc)
	}
	if count == 0 {
		return nil, nil
	}
	n := int(count)
	d, err := devAlloc(4 * n)
	if err != nil {
		return nil, err
	}
	defer d.free()
	if rc := C.gpd_flow_expire(t.ft, C.uint64_t(olderThanSeq), dhold, flags, (*C.uint32_t)(d.p), C.uint64_t(n), &count,
		nil); rc != C.GPD_OK {
		return nil, lastError("gpd_flow_expire", rc)
	}
	out := make([]uint32, int(count))
	if err := fromDev(unsafe.Pointer(&out[0]), d, 4*int(count)); err != nil {
		return nil, err
	}
	return out, nil
}

// Hold is Expire's hold mask for this assembler: one byte per flow record, non-zero where the
// connection is open or holds pages.  A closed connection's state is all zero already, so the
// records Expire removes need nothing returned to the fresh state here.
func (a *Assembler) Hold() ([]uint8, error) {
	conns, err := a.Conns()
	if err != nil {
		return nil, err
	}
	hold := make([]uint8, len(conns))
	for k, c := range conns {
		if c.Flags != 0 || c.Pages != 0 {
			hold[k] = 1
		}
	}
	return hold, nil
}

// Load returns the records in use and the tombstones: removed slots that no sweep could turn
// empty yet, because a record sits behind them on its probe chain.
func (t *FlowTable) Load() (used, tombstones uint64, err error) {
	done, err := t.parser.onDevice()
	if err != nil {
		return 0, 0, err
	}
	defer done()
	var out [2]C.uint64_t
	if rc := C.gpd_flow_load(t.ft, &out[0], nil); rc != C.GPD_OK {
		return 0, 0, lastError("gpd_flow_load", rc)
	}
	return uint64(out[0]), uint64(out[1]), nil
}
