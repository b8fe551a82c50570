// host_error.h -- the message of a library's last failure: one buffer per translation unit that includes this (each JPEG library
// is one translation unit, so each has its own), written by fail() and handed out by the library's *_last_error().
// Not thread-local, as the headers under include/ document (mdct_api.hip's thread-local pair is a different contract).
#pragma once
#include <stdarg.h>
#include <stdio.h>

namespace
{
char g_err[512];

int fail(int code, const char *fmt, ...)
{
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}
} // namespace
