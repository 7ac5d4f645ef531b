// CPython extension `open_spiel_amd._osg_step_fast`: StateBatch.step's argument checks and its osg_step call as one
// METH_FASTCALL function.  At 2^20 connect_four states the fused step kernel lasts about as long as a copy of its
// bytes, so what a back-to-back launch costs is set by the host code that issues it: three Python tensor checks and a
// ctypes call took several microseconds per launch, these checks take nanoseconds.
//
// The checks are those of StateBatch._checked (engine.py): a torch tensor, uint8, on the context's device, strided
// and contiguous, exactly `numel` elements.  Nothing is cached by tensor identity (resize_ / set_ keep the identity).
// osg_step stays the only place that chooses a kernel: it is called through the address ctypes resolved in the library
// engine.py loaded (bind()), so that the handles and the code they are used with come from the same library — also
// under OSG_VARIANT_LIB.
#define PY_SSIZE_T_CLEAN
#include <Python.h>

#include <torch/csrc/autograd/python_variable.h>

#include <cstdint>

namespace {

using step_fn = int (*)(const void* src, void* dst, const uint8_t* d_actions, void* d_mask, uint8_t* d_status);
using last_error_fn = const char* (*)();

step_fn g_step = nullptr;
last_error_fn g_last_error = nullptr;
PyObject* g_error = nullptr;        // open_spiel_amd.OsgError
PyObject* g_bad_tensor = nullptr;   // engine._bad_tensor_message(t, dtype, numel, what, device) -> str
PyObject* g_uint8 = nullptr;        // torch.uint8
PyObject* g_device_ctor = nullptr;  // torch.device

bool tensor_ok(PyObject* o, int64_t numel, int device) {
  if (!THPVariable_Check(o)) return false;
  const at::Tensor& t = THPVariable_Unpack(o);
  return t.scalar_type() == at::kByte && t.is_cuda() && t.get_device() == device && t.layout() == at::kStrided &&
         t.is_contiguous() && t.numel() == numel;
}

// The OsgError _checked raises for the same tensor, with its text (the cold path: formatted by engine.py).
PyObject* raise_bad_tensor(PyObject* t, int64_t numel, const char* what, int device) {
  PyObject* dev = PyObject_CallFunction(g_device_ctor, "si", "cuda", device);
  if (!dev) return nullptr;
  PyObject* msg = PyObject_CallFunction(g_bad_tensor, "OOLsO", t, g_uint8, static_cast<long long>(numel), what, dev);
  Py_DECREF(dev);
  if (!msg) return nullptr;
  PyErr_SetObject(g_error, msg);
  Py_DECREF(msg);
  return nullptr;
}

// bind(OsgError, bad_tensor_message, torch.uint8, torch.device, address of osg_step, address of osg_last_error)
PyObject* bind(PyObject*, PyObject* args) {
  PyObject *error, *bad_tensor, *uint8, *device_ctor;
  unsigned long long step_addr, last_error_addr;
  if (!PyArg_ParseTuple(args, "OOOOKK", &error, &bad_tensor, &uint8, &device_ctor, &step_addr, &last_error_addr))
    return nullptr;
  if (!step_addr || !last_error_addr) {
    PyErr_SetString(PyExc_ValueError, "bind: NULL function address");
    return nullptr;
  }
  Py_INCREF(error);
  Py_INCREF(bad_tensor);
  Py_INCREF(uint8);
  Py_INCREF(device_ctor);
  Py_XSETREF(g_error, error);
  Py_XSETREF(g_bad_tensor, bad_tensor);
  Py_XSETREF(g_uint8, uint8);
  Py_XSETREF(g_device_ctor, device_ctor);
  g_step = reinterpret_cast<step_fn>(static_cast<uintptr_t>(step_addr));
  g_last_error = reinterpret_cast<last_error_fn>(static_cast<uintptr_t>(last_error_addr));
  Py_RETURN_NONE;
}

PyObject* bound(PyObject*, PyObject*) { return PyBool_FromLong(g_step != nullptr); }

// step(src_h, dst_h, n, dst_n, game, dst_game, actions, mask, status, compact_mask_bytes, device) -> None
//   src_h / dst_h: osg_batch* as int (0 = closed); mask: None = do not write it (want_mask=False); device: CUDA index.
// Checks in the order StateBatch._step_py makes them, then osg_step.
PyObject* step(PyObject*, PyObject* const* args, Py_ssize_t nargs) {
  if (nargs != 11) {
    PyErr_SetString(PyExc_TypeError, "step: expected 11 arguments");
    return nullptr;
  }
  if (!g_step) {
    PyErr_SetString(PyExc_RuntimeError, "step: bind() was not called");
    return nullptr;
  }
  void* src = PyLong_AsVoidPtr(args[0]);
  void* dst = PyLong_AsVoidPtr(args[1]);
  const long long n = PyLong_AsLongLong(args[2]);
  const long long dst_n = PyLong_AsLongLong(args[3]);
  const long cmb = PyLong_AsLong(args[9]);
  const long device = PyLong_AsLong(args[10]);
  if (PyErr_Occurred()) return nullptr;
  PyObject* actions = args[6];
  PyObject* mask = args[7];
  PyObject* status = args[8];

  if (!src || !dst) {
    PyErr_SetString(g_error, "step: the batch or its destination is closed");
    return nullptr;
  }
  if (mask != Py_None && !tensor_ok(mask, n * cmb, static_cast<int>(device)))
    return raise_bad_tensor(mask, n * cmb, "step(mask=)", static_cast<int>(device));
  if (!tensor_ok(status, n, static_cast<int>(device)))
    return raise_bad_tensor(status, n, "step(status=)", static_cast<int>(device));
  if (!tensor_ok(actions, n, static_cast<int>(device)))
    return raise_bad_tensor(actions, n, "step(actions_u8)", static_cast<int>(device));
  int same = dst_n == n ? PyObject_RichCompareBool(args[4], args[5], Py_EQ) : 0;
  if (same < 0) return nullptr;
  if (!same) {
    PyErr_SetString(g_error, "step(dst=): destination batch of a different game or size");
    return nullptr;
  }

  const auto* d_actions = static_cast<const uint8_t*>(THPVariable_Unpack(actions).data_ptr());
  void* d_mask = mask == Py_None ? nullptr : THPVariable_Unpack(mask).data_ptr();
  auto* d_status = static_cast<uint8_t*>(THPVariable_Unpack(status).data_ptr());
  int rc;
  Py_BEGIN_ALLOW_THREADS  // as ctypes does around a foreign call: a launch may wait for room in a full queue
  rc = g_step(src, dst, d_actions, d_mask, d_status);
  Py_END_ALLOW_THREADS
  if (rc != 0) return PyErr_Format(g_error, "osg error %d: %s", rc, g_last_error());
  Py_RETURN_NONE;
}

PyMethodDef kMethods[] = {
    {"bind", bind, METH_VARARGS, "bind(OsgError, bad_tensor_message, torch.uint8, torch.device, osg_step, osg_last_error)"},
    {"bound", bound, METH_NOARGS, "True once bind() has been called"},
    {"step", reinterpret_cast<PyCFunction>(reinterpret_cast<void (*)(void)>(step)), METH_FASTCALL,
     "step(src_h, dst_h, n, dst_n, game, dst_game, actions, mask, status, compact_mask_bytes, device)"},
    {nullptr, nullptr, 0, nullptr}};

PyModuleDef kModule = {PyModuleDef_HEAD_INIT, "_osg_step_fast", "StateBatch.step's checks and osg_step call", -1,
                       kMethods, nullptr, nullptr, nullptr, nullptr};

}  // namespace

PyMODINIT_FUNC PyInit__osg_step_fast() { return PyModule_Create(&kModule); }
