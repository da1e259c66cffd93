/* Stands in for GLEW when the reference's host sources are compiled for oracle/_ref/ref_host:
   the system GL headers declare every gl*Buffer* entry point those sources name. */
#define GL_GLEXT_PROTOTYPES 1
#include <GL/gl.h>
#include <GL/glext.h>
