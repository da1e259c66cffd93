/* Link-only stand-ins for the GL and CUDA entry points that the reference's host sources leave
   undefined in oracle/_ref/ref_host. Written from the linker's list of undefined symbols; they
   compute nothing. Every one prints its name and aborts, so a path of ref_driver.cc that reached
   a GPU or GL call dies loudly and no value made here can reach a byte that a test compares.

   The exceptions, each with the call site that needs it. They act on host memory that the
   driver never reads back: the reference keeps its own host copy of every buffer (m_nodes,
   m_triWoop, m_triIndex, the pixel tables) and serialises that copy.
     cudaMalloc  CudaBVH.cc:90-92 (stream constructor), :350-352 (createCompact),
                 PixelTable.cc:72-73: malloc()
     cudaMemcpy  CudaBVH.cc:94-96, :354-356, PixelTable.cc:158-159: memcpy() into that block
     cudaFree    CudaBVH.cc:105-107 (destructor), PixelTable.cc:48-49: free()
   Nothing else is called: Buffer keeps its data on the CPU side until someone asks for a CUDA or
   GL pointer (nobody does), and CudaModule::staticInit, the only caller of cuInit, never runs. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define ABORTING(name) int name() { fprintf(stderr, "ref_shim: %s called\n", #name); abort(); }

ABORTING(glBindBuffer)
ABORTING(glBufferData)
ABORTING(glBufferSubData)
ABORTING(glDeleteBuffers)
ABORTING(glGenBuffers)
ABORTING(glGetBufferParameteriv)
ABORTING(glGetBufferSubData)
ABORTING(glGetIntegerv)

ABORTING(cuInit)
ABORTING(cuGLMapBufferObject_v2)
ABORTING(cuGLRegisterBufferObject)
ABORTING(cuGLUnmapBufferObject)
ABORTING(cuGLUnregisterBufferObject)
ABORTING(cuMemAllocHost_v2)
ABORTING(cuMemAlloc_v2)
ABORTING(cuMemFreeHost)
ABORTING(cuMemFree_v2)
ABORTING(cuMemcpyDtoDAsync_v2)
ABORTING(cuMemcpyDtoD_v2)
ABORTING(cuMemcpyDtoHAsync_v2)
ABORTING(cuMemcpyDtoH_v2)
ABORTING(cuMemcpyHtoDAsync_v2)
ABORTING(cuMemcpyHtoD_v2)
ABORTING(cuMemsetD8_v2)

ABORTING(cudaGetErrorString)

/* The three exceptions; 0 is "no error" to cutilSafeCall. */
int cudaMalloc(void** p, size_t n)
{
    *p = malloc(n ? n : 1);
    if (!*p)
        abort();
    return 0;
}

int cudaMemcpy(void* dst, const void* src, size_t n, int kind)
{
    (void)kind;
    memcpy(dst, src, n);
    return 0;
}

int cudaFree(void* p)
{
    free(p);
    return 0;
}
